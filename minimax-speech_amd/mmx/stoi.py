"""Short-time objective intelligibility (STOI) and extended STOI of an estimate against a reference on the device: what the
reference's `audiotools.metrics.quality.stoi(estimates, references, extended=False)` (dac-vae/audiotools/metrics/quality.py:9-61)
asks the host library `pystoi` for, one clip at a time.  Here: a ragged batch in four launches of csrc/stoi.hip (mmx_stoi_select,
mmx_stoi_bands, mmx_stoi_score) after at most one resample launch per signal, without a host sync, atomics or a spectrogram in
memory.  pystoi, audiotools and scipy are not dependencies (restated seams): the definition below is restated from
the published algorithm (Taal, Hendriks, Heusdens, Jensen 2011; Jensen, Taal 2016) as that library implements it.  It has NOT
been compared against pystoi itself, which is not available where this was built; tests/stoi_f64.py is a float64 restatement of
the same text and the yardstick of the tests.

Definition.  FS = 10000, frames of 256 samples at hop 128, NFFT = 512, 15 third-octave bands from 150 Hz, segments of N = 30
frames, BETA = -15 dB, dynamic range 40 dB, EPS = 2^-52.  x the reference (clean), y the estimate, equal length, at 10 kHz;
w = numpy.hanning(258)[1:-1].
 1. Frames start at i = 0, 128, .. with i < n - 256 (strict): ceil((n - 256) / 128) frames.  Steps 2 and 3 both frame this way.
 2. Silent frames: e_i = 20 log10(|w x[i : i + 256]| + EPS) on the reference; frame i is kept iff max(e) - 40 - e_i < 0.  With F
    kept frames, in order, both signals are rebuilt by overlap-add of their own windowed kept frames at hop 128 to
    (F - 1) * 128 + 256 samples (the window is applied here and once more in step 3, as the library does).
 3. X = rfft(w xs[i : i + 256], 512) over the frames of the rebuilt signal: F - 1 of them, the strict bound of rule 1 again.
 4. Bands: f = linspace(0, 10000, 513)[:257]; band k holds the bins [argmin (f - lo)^2, argmin (f - hi)^2) with
    lo = 150 * 2^((2k - 1) / 6), hi = 150 * 2^((2k + 1) / 6): BAND_EDGES below.  Xb = sqrt(OBM |X|^2), the same for Y.
 5. Fewer than 30 spectral frames: the result is 1e-5 (the library's value, with a warning there; here `return_frames` reports
    the count).
 6. Standard: for each segment m = 30 .. frames (columns m - 30 .. m - 1) and band: c = |x_seg| / (|y_seg| + EPS),
    y' = min(c y_seg, x_seg (1 + 10^(15/20))); subtract the means of y' and x_seg, divide each by its norm + EPS, sum the
    products; d = the mean over the J * 15 (segment, band) pairs.
 7. extended=True: for each segment (15 x 30): remove the row means and normalise the rows (norm + EPS), then the same over the
    columns; d = sum(x^ y^) / 30 / J.
 8. Other sample rates: both clips first go through this project's own sinc resampler (mmx.resample) to 10 kHz.  pystoi uses a
    different polyphase filter there, so a number from, say, a 24 kHz pair is STOI on THIS PROJECT'S 10 kHz rendering and would not
    match pystoi's bit for bit even where steps 1 - 7 do.

On the device steps 2 - 5 run in fp32 (energies: fp32 products, fp64 sums; spectra and band sums: the six-term bf16 MFMA products
of csrc/spec_tile.h, fp32 accumulation) and steps 6 - 7 in fp64 from the fp32 band envelopes, summed in a fixed order: a clip's
result is that of its solo run, bit for bit.  There is no CPU fallback: a CPU tensor raises MmxError."""
import numpy as np
import torch

from . import clips as CL
from . import mel as MEL
from . import ops
from ._lib import MmxError, call, stream, _p
from .resample import Resample

FS, FRAME, HOP, NFFT, BANDS, SEG = 10000, 256, 128, 512, 15, 30
MIN_FREQ, BETA, DYN_RANGE, EPS = 150.0, -15.0, 40.0, 2.0 ** -52
TOO_SHORT = 1e-5                                         # the library's value for fewer than SEG spectral frames
BAND_EDGES = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
              (109, 138), (138, 174), (174, 219))
FRAMES_PER_TILE, SEGMENTS_PER_TILE, GAP, BIN_TILES = 16, 16, 16, 14      # csrc/stoi.hip: spec_tile.h's frame tile, SC_SEGS, ST_GAP, ST_BT


def frames_of(n):
    """Frames of a clip of n samples (rule 1): starts 0, 128, .. strictly below n - 256."""
    return -(-(int(n) - FRAME) // HOP) if n > FRAME else 0


def spectral_frames(kept):
    """Frames of the signal that `kept` kept frames rebuild: frames_of((kept - 1) * 128 + 256) = kept - 1."""
    return max(int(kept) - 1, 0)


def padded_bins():
    return ops.round_up(NFFT // 2 + 1, 32)


def window():
    """float64 [256]: numpy.hanning(258)[1:-1]."""
    return np.hanning(FRAME + 2)[1:-1]


def band_edges():
    """[(first bin, one past the last bin)] of the 15 third-octave bands over the 257 bins of a 512-point DFT at 10 kHz (rule 4)."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(BANDS, dtype=np.float64)
    lo, hi = MIN_FREQ * 2.0 ** ((2 * k - 1) / 6), MIN_FREQ * 2.0 ** ((2 * k + 1) / 6)
    return [(int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi)]


def third_octave_table():
    """float64 [16, padded_bins(512)]: the 0 / 1 band matrix, one zero row and zero columns of padding."""
    t = torch.zeros(16, padded_bins(), dtype=torch.float64)
    for k, (a, b) in enumerate(band_edges()):
        t[k, a:b] = 1.0
    return t


def dft_basis():
    """float64 [2 * padded_bins, 256]: mel.dft_basis of the 512-point DFT with the window followed by 256 zeros, cut to the 256
    columns that are not zero (the others add exact zeros to every sum)."""
    w = np.concatenate([window(), np.zeros(NFFT - FRAME)])
    return MEL.dft_basis(NFFT, 0, NFFT // 2 + 1, window=w)[:, :FRAME]


def lds_bytes():
    """Dynamic LDS of stoi_bands_kernel (ST_LDS of csrc/stoi.hip): the sample planes of 16 frames of both signals (three bf16 planes
    each, hop-sized chunks GAP apart) and their |X|^2 planes [3][16][16 * BIN_TILES + 8]."""
    span = (FRAMES_PER_TILE - 1) * HOP + FRAME
    return 2 * 3 * 2 * (span + GAP * -(-span // HOP)) + 2 * 3 * 16 * (16 * BIN_TILES + 8) * 2


def refusal(lens, sample_rate=FS, est_lens=None):
    """Why stoi refuses these reference clip lengths (at 10 kHz), this rate, or these estimate lengths: nothing is launched then.
    None where it takes them."""
    if not (isinstance(sample_rate, (int, np.integer)) or float(sample_rate).is_integer()) or sample_rate < 1:
        return f"sample rate {sample_rate} is not a positive whole number of Hz"
    lens = [int(v) for v in lens]
    if est_lens is not None and [int(v) for v in est_lens] != lens:
        return f"estimate and reference clips differ in length: {[int(v) for v in est_lens]} against {lens}"
    short = [v for v in lens if v <= FRAME]
    if short:
        return f"a clip of {short[0]} samples at {FS} Hz holds no frame of {FRAME} samples"
    return None


def _device_tables(dev):
    """(basis planes, band-table planes, fp32 window) on `dev`, built once per device."""
    def build():
        assert band_edges()[-1][1] <= 16 * BIN_TILES
        return (MEL.packed3(dft_basis(), dev), MEL.packed3(third_octave_table(), dev),
                torch.from_numpy(window().astype(np.float32)).to(dev))
    return CL.device_tables(("stoi", str(dev)), build)


def _refuse(what, x, lens):
    CL.on_device(what, x)
    why = refusal(lens or [x.shape[1]])
    if why:
        raise MmxError(f"{what}: {why}")


def select(ref, lens=None, d_lens=None, h_lens=None):
    """Rule 2's decision for references fp32 [B, L] at 10 kHz on the device -> dict(energy f64 [B, cap], mask uint8 [B, cap],
    map int32 [B, cap] (source frame of kept frame i; -1 from F on), kept int32 [B], cap = frames_of(L))."""
    _refuse("mmx_stoi_select", ref, lens)
    B, L = ref.shape
    if d_lens is None:
        d_lens, h_lens = CL.lens_args(lens, L, ref.device)
    _, _, win = _device_tables(ref.device)
    cap = frames_of(L)
    out = dict(energy=torch.zeros(B, cap, dtype=torch.float64, device=ref.device), mask=torch.empty(B, cap, dtype=torch.uint8, device=ref.device),
               map=torch.empty(B, cap, dtype=torch.int32, device=ref.device), kept=torch.empty(B, dtype=torch.int32, device=ref.device), cap=cap)
    call("mmx_stoi_select", _p(ref), CL.row_stride(ref), L, B, _p(d_lens), h_lens, _p(win), _p(out["energy"]), _p(out["mask"]),
         _p(out["map"]), _p(out["kept"]), cap, stream())
    return out


def bands(est, ref, lens, sel, d_lens=None, h_lens=None):
    """Rules 2 - 4 after the decision: est, ref fp32 [B, L] on the device and select()'s result -> the band envelopes fp32
    [B, 2, cap, 16] (signal 0 the reference, 1 the estimate; column 15 and the rows from kept - 1 on are zero)."""
    _refuse("mmx_stoi_bands", est, lens)
    _refuse("mmx_stoi_bands", ref, lens)
    B, L = ref.shape
    if d_lens is None:
        d_lens, h_lens = CL.lens_args(lens, L, ref.device)
    basis, filt, win = _device_tables(ref.device)
    cap = sel["cap"]
    env = torch.zeros(B, 2, cap, 16, dtype=torch.float32, device=ref.device)
    call("mmx_stoi_bands", _p(est), CL.row_stride(est), _p(ref), CL.row_stride(ref), L, B, _p(d_lens), h_lens, _p(win), _p(sel["map"]),
         _p(sel["kept"]), _p(basis), _p(filt), _p(env), cap, stream())
    return env


def score(env, kept, extended=False):
    """Rules 5 - 7: envelopes [B, 2, cap, 16] and the kept counts -> (d f64 [B], spectral frames int32 [B])."""
    B, _, cap, _ = env.shape
    wcap = max(1, -(-(cap - SEG) // SEGMENTS_PER_TILE))
    work = torch.empty(B, wcap, dtype=torch.float64, device=env.device)
    out = torch.empty(B, dtype=torch.float64, device=env.device)
    frames = torch.empty(B, dtype=torch.int32, device=env.device)
    call("mmx_stoi_score", _p(env), cap, B, _p(kept), int(bool(extended)), _p(work), wcap, _p(out), _p(frames), stream())
    return out, frames


@torch.no_grad()
def stoi(est, ref, sample_rate, extended=False, lens=None, return_frames=False):
    """STOI (extended=True: extended STOI) of each estimate against its reference: two lists of mono clips or two padded tensors
    [B, L] / [B, 1, L] with `lens`, at `sample_rate` Hz -> f64 [B] on the device; with return_frames also the spectral frame counts
    int32 [B] (below 30: the value is 1e-5, as the library returns with a warning).  Rates other than 10 kHz go through this
    project's own resampler first (one launch per signal): such a number is STOI on this project's 10 kHz rendering, not a bit-match
    of a library that resamples with another filter (rule 8 above).  MmxError where refusal() gives a reason: nothing is launched
    then.  Nothing is read back; a clip's value is that of its solo run, bit for bit."""
    why = refusal([FRAME + 1], sample_rate)
    if why:
        raise MmxError(f"stoi: {why}")
    x, y, lens = CL.pack_pair(est, ref, lens, "stoi")    # x the estimate, y the reference; ValueError where the lengths differ
    CL.on_device("stoi", x, y)
    rate = int(sample_rate)
    if rate != FS:
        rs = Resample(rate, FS)
        x, y = rs(x, lens), rs(y, lens)
        lens = [rs.out_len(n) for n in lens]
    why = refusal(lens)
    if why:
        raise MmxError(f"stoi: {why}")
    d_lens, h_lens = CL.lens_args(lens, x.shape[1], x.device)
    sel = select(y, lens, d_lens, h_lens)
    d, frames = score(bands(x, y, lens, sel, d_lens, h_lens), sel["kept"], extended)
    return (d, frames) if return_frames else d


class STOI(torch.nn.Module):
    """quality.stoi as a module with tensors in place of AudioSignal: forward(estimates, references, lens=None) -> f64 [B]."""

    def __init__(self, sample_rate: int = FS, extended: bool = False):
        super().__init__()
        self.sample_rate, self.extended = int(sample_rate), bool(extended)

    def forward(self, estimates, references, lens=None):
        return stoi(estimates, references, self.sample_rate, extended=self.extended, lens=lens)
