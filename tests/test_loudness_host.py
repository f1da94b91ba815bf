"""Host side of the loudness meter (mmx/loudness.py): coefficients, block counts, the state-transition tables the kernel is handed
and the guards, without a GPU, against a float64 yardstick written here from the definition in that module's docstring
(ITU-R BS.1770-4 as pyloudnorm / audiotools implement it): scipy.signal.lfilter in float64 and a plain loop over the blocks.  The
yardstick knows nothing of segments, sub-blocks or the scan.  tests/test_gpu_loudness.py measures the kernels against
`loudness_f64` of this file on the clips of `fixture_clips`.

A fixture clip is DECIDED: in float64 no block's loudness is within 0.05 dB of a gate (-70 or Gamma_r), so the set of kept blocks
is a property of the clip and not of the last bits of an energy sum.  A clip that fails this is a bad fixture, not a tolerated
case."""
import math
import os
import re

import numpy as np
import pytest
import scipy.signal
import torch

from mmx import loudness as LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (16000, 22050, 24000, 44100, 48000)
G = np.array([1.0, 1.0, 1.0, 1.41, 1.41])
DECIDED_DB = 0.05


# ------------------------------------------------------------------------------------------------ the float64 yardstick
def kw_f64(rate):
    """[(b, a) high shelf, (b, a) high pass], float64, a[0] = 1: pyloudnorm's IIRfilter formulas."""
    out = []
    for kind, Gdb, Q, fc in (("shelf", 4.0, 1.0 / np.sqrt(2.0), 1500.0), ("hp", 0.0, 0.5, 38.0)):
        A = 10.0 ** (Gdb / 40.0)
        w0 = 2.0 * np.pi * (fc / rate)
        al = np.sin(w0) / (2.0 * Q)
        c = np.cos(w0)
        if kind == "shelf":
            b = [A * ((A + 1) + (A - 1) * c + 2 * np.sqrt(A) * al), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - 2 * np.sqrt(A) * al)]
            a = [(A + 1) - (A - 1) * c + 2 * np.sqrt(A) * al, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - 2 * np.sqrt(A) * al]
        else:
            b, a = [(1 + c) / 2, -(1 + c), (1 + c) / 2], [1 + al, -2 * c, 1 - al]
        out.append((np.array(b, dtype=np.float64) / a[0], np.array(a, dtype=np.float64) / a[0]))
    return out


def k_filter(x, rate, dtype=np.float64, fir=0):
    """x [nt, nch] float64 -> the K-weighted signal, float64.  dtype=np.float32: lfilter runs on float32 arrays (what the
    reference's CPU path computes).  fir=N: each section replaced by the first N samples of its impulse response (the reference's
    GPU path, zeros=N)."""
    y = x
    for b, a in kw_f64(rate):
        if fir:
            imp = np.zeros(fir)
            imp[0] = 1.0
            h = scipy.signal.lfilter(b, a, imp)
            y = np.stack([np.convolve(y[:, c], h)[:y.shape[0]] for c in range(y.shape[1])], axis=1)
        else:
            y = scipy.signal.lfilter(b.astype(dtype), a.astype(dtype), y.astype(dtype), axis=0).astype(np.float64)
    return y


def loudness_f64(x, rate, partial="pad", dtype=np.float64, fir=0):
    """x [nt] or [nt, nch] -> dict(lufs, l [F], keep bool [F], gamma_r, F).  lufs is floored at -70."""
    x = np.asarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    n = x.shape[0]
    if n / rate < 0.5:
        x = np.concatenate([x, np.zeros((int((0.5 - n / rate) * rate), x.shape[1]))], axis=0)
        n = x.shape[0]
    nch = x.shape[1]
    y = k_filter(x, rate, dtype, fir)
    K, S = int(0.4 * rate), int(0.4 * rate * 0.25)
    F = (n - K) // S + 1 if partial == "drop" else int(math.ceil((max(n, K) - K) / S)) + 1
    z = np.zeros((nch, max(F, 0)))
    for j in range(F):
        blk = y[j * S:j * S + K]                                # the tail block is short: its missing samples are zeros
        z[:, j] = (blk * blk).sum(axis=0) / (0.4 * rate)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10((G[:nch, None] * z).sum(axis=0))
        k1 = l > -70.0
        if not k1.any():
            return dict(lufs=-70.0, l=l, keep=np.zeros(max(F, 0), dtype=bool), gamma_r=None, F=F)
        gamma_r = -0.691 + 10.0 * np.log10((G[:nch] * z[:, k1].mean(axis=1)).sum()) - 10.0
        keep = k1 & (l > gamma_r)
        lufs = -0.691 + 10.0 * np.log10((G[:nch] * z[:, keep].mean(axis=1)).sum()) if keep.any() else -70.0
    return dict(lufs=max(float(lufs), -70.0), l=l, keep=keep, gamma_r=float(gamma_r), F=F)


# ------------------------------------------------------------------------------------------------ fixtures (shared with the GPU test)
def tone_clip(rate, seed):
    """2.3 s (55 200 samples at 24 kHz): 0.9 s at -40 dB, then noise plus a 0.3-amplitude 60 Hz tone.  The lead-in is noise at
    -40 dB re full scale (sigma 0.01, the noise floor of the rest), its first 0.45 s another 40 dB down, so that both gates are
    at work: blocks below -70, blocks between -70 and Gamma_r, blocks kept.  Several sub-blocks and low-frequency content."""
    rng = np.random.default_rng(seed)
    n, nq = round(2.3 * rate), round(0.9 * rate)
    noise = 0.01 * rng.standard_normal(n)
    x = noise + 0.3 * np.sin(2.0 * np.pi * 60.0 * np.arange(n) / rate)
    x[:nq] = noise[:nq]
    x[:nq // 2] *= 0.01
    return x.astype(np.float32)


def noise_clip(n, seed, sigma=0.1):
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


_CLIPS = None


def fixture_clips():
    """name -> (rate, float32 samples).  Built once and never modified."""
    global _CLIPS
    if _CLIPS is None:
        _CLIPS = {"n7200": (24000, noise_clip(7200, 1)), "n9600": (24000, noise_clip(9600, 2)), "n9601": (24000, noise_clip(9601, 3)),
                  "n12000": (24000, noise_clip(12000, 4)), "n13001": (24000, noise_clip(13001, 8)), "tone24k": (24000, tone_clip(24000, 5)),
                  "zeros": (24000, np.zeros(12000, dtype=np.float32)),
                  "tone16k": (16000, tone_clip(16000, 6)), "tone48k": (48000, tone_clip(48000, 7))}
        for _, x in _CLIPS.values():
            x.setflags(write=False)
    return _CLIPS


_REF = {}


def reference(name, partial="pad"):
    """The yardstick's result for a fixture clip, computed once."""
    if (name, partial) not in _REF:
        rate, x = fixture_clips()[name]
        _REF[(name, partial)] = loudness_f64(x, rate, partial)
    return _REF[(name, partial)]


# ------------------------------------------------------------------------------------------------ tests
def test_k_weighting_is_the_bs1770_table_at_48k():
    """The table's `a` of both sections to 1e-4 absolute.  The shelf's `b` to 1e-4 of each coefficient: pyloudnorm's closed form
    (G = 4, Q = 1/sqrt 2, fc = 1500) is a rounded parametrisation of the table's filter, and its b[1] = -2.691804 sits 1.08e-4
    (4.0e-5 of its value) from the table's -2.691696; the 997 Hz test below is what bounds the consequence."""
    (b1, a1), (b2, a2) = LD.k_weighting(48000)
    tb1 = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285])
    assert np.abs((b1 - tb1) / tb1).max() < 1e-4
    assert np.abs(a1 - [1.0, -1.69065929318241, 0.73248077421585]).max() < 1e-4
    assert np.abs(a2 - [1.0, -1.99004745483398, 0.99007225036621]).max() < 1e-4
    for rate in RATES:                                          # the module's coefficients are the yardstick's
        for (b, a), (rb, ra) in zip(LD.k_weighting(rate), kw_f64(rate)):
            assert b.dtype == np.float64 and np.abs(b - rb).max() < 1e-15 and np.abs(a - ra).max() < 1e-15 and a[0] == 1.0
        # passband gain 1: the shelf at dc, the high pass at the Nyquist frequency
        (b1, a1), (b2, a2) = LD.k_weighting(rate)
        assert abs(b1.sum() / a1.sum() - 1.0) < 1e-12 and abs((b2[0] - b2[1] + b2[2]) / (a2[0] - a2[1] + a2[2]) - 1.0) < 1e-12


@pytest.mark.parametrize("rate", [16000, 24000, 44100, 48000])
def test_full_scale_997hz_sine_measures_minus_3_01(rate):
    """EBU Tech 3341's meter tolerance, 0.1 LU, through the yardstick; two channels measure 3.01 dB above one."""
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(3 * rate) / rate)
    mono = loudness_f64(x, rate)["lufs"]
    assert abs(mono - (-3.01)) <= 0.1, mono
    stereo = loudness_f64(np.stack([x, x], axis=1), rate)["lufs"]
    assert abs(stereo - mono - 10.0 * np.log10(2.0)) < 1e-6
    assert LD.block_sizes(rate) == (int(0.4 * rate), int(0.1 * rate))


@pytest.mark.parametrize("rate", RATES)
def test_block_counts_of_pad_and_drop(rate):
    K, S = LD.block_sizes(rate)
    assert K == 4 * S
    want = {"pad": [1, 1, 2, 2, 3], "drop": [0, 1, 1, 2, 2]}
    for partial in ("pad", "drop"):
        ns = [K - 1, K, K + 1, K + S, K + S + 1]
        assert [LD.n_blocks(n, rate, partial) for n in ns] == want[partial]
        # the kernel's rule, in sub-blocks of S after the 0.5 s rule: ceil(n' / S) or n' // S of them, three fewer blocks
        for n in ns + [1, S, 3 * S + 7, 17 * S - 1, 17 * S]:
            n_ = LD.padded_len(n, rate)
            assert n_ >= K and n_ <= max(n, rate // 2 + 1)
            nsub = n_ // S if partial == "drop" else -(-n_ // S)
            assert nsub - 3 == LD.n_blocks(n_, rate, partial) == loudness_f64(np.zeros(n), rate, partial)["F"]
            assert nsub <= LD._cap(n, rate, S)


@pytest.mark.parametrize("rate", RATES)
def test_transition_tables_reproduce_lfilter_across_boundaries(rate):
    """What the kernel is handed: the state a run reaches is (power of A) x (state before) + (state the run reaches from zero).
    Checked against scipy.signal.lfilter's own zi / zf in float64, to 1e-12: across a segment boundary with A^seg, over the scan's
    strides with A^(seg 2^k), across a sub-block with A^S (1e-10: see there)."""
    tab, seg = LD.tables(rate)
    K, S = LD.block_sizes(rate)
    assert tab.dtype == np.float64 and tab.shape == (10 + 16 * 8,) and S % seg == 0 and S // seg <= 127 and seg <= 64
    (b1, a1), (b2, a2) = kw_f64(rate)
    assert np.abs(tab[:10] - np.concatenate([b1, a1[1:], b2, a2[1:]])).max() < 1e-15
    P = [tab[10 + 16 * k:26 + 16 * k].reshape(4, 4) for k in range(8)]

    def run(x, s):
        y1, z1 = scipy.signal.lfilter(b1, a1, x, zi=s[:2])
        y2, z2 = scipy.signal.lfilter(b2, a2, y1, zi=s[2:])
        return y2, np.concatenate([z1, z2])

    rng = np.random.default_rng(rate)
    x = rng.standard_normal(3 * seg)
    y, end = run(x, np.zeros(4))
    s1 = run(x[:seg], np.zeros(4))[1]
    s2 = P[0] @ s1 + run(x[seg:2 * seg], np.zeros(4))[1]
    y3, e3 = run(x[2 * seg:], s2)
    assert np.abs(y3 - y[2 * seg:]).max() < 1e-12 and np.abs(e3 - end).max() < 1e-12
    # the scan's longer strides and the carry across a sub-block, at the output: a state reached through A^(seg 2^k) or A^S
    # continues the signal as lfilter's own state does.  The high pass keeps two large, nearly opposite states (a double pole at
    # 0.985 .. 0.995: ~100 for this unit-variance input) which these matrices (entries ~30) multiply, so one product already rounds
    # at 4 * 30 * 100 * 2^-53 = 1e-12, and lfilter's run of up to 4800 steps rounds as well: 1e-10, seven orders below the meter's bound
    for k, n in [(k, seg << k) for k in range(1, 7)] + [(7, S)]:
        x = rng.standard_normal(seg + n + seg)
        y, _ = run(x, np.zeros(4))
        sa = run(x[:seg], np.zeros(4))[1]
        sb = P[k] @ sa + run(x[seg:seg + n], np.zeros(4))[1]
        assert np.abs(run(x[seg + n:], sb)[0] - y[seg + n:]).max() < 1e-10, (k, n)
    # a whole sub-block boundary with input on both sides
    x = rng.standard_normal(2 * S)
    y, _ = run(x, np.zeros(4))
    y2, _ = run(x[S:], P[7] @ np.zeros(4) + run(x[:S], np.zeros(4))[1])
    assert np.abs(y2 - y[S:]).max() < 1e-12                     # (a zero state before: lfilter's own zf, untouched by the table)


def test_guards():
    for rate in (11025, 12345, 0, -5):
        with pytest.raises(ValueError):
            LD.block_sizes(rate)
        with pytest.raises(ValueError):
            LD.Meter(rate)
    with pytest.raises(ValueError):
        LD.tables(11025)
    with pytest.raises(NotImplementedError):
        LD.Meter(24000, filter_class="Fenton/Lee 1")
    with pytest.raises(NotImplementedError):
        LD.Meter(24000, block_size=0.2)
    m = LD.Meter(24000, zeros=256, use_fir=True)                # accepted, ignored: the exact filters run
    assert (m.rate, m.partial, m.G) == (24000, "pad", [1.0, 1.0, 1.0, 1.41, 1.41])
    with pytest.raises(LD.MmxError):
        m.integrated_loudness(torch.zeros(1, 12000, 1))
    with pytest.raises(LD.MmxError):
        LD.integrated_loudness([torch.zeros(12000)], 24000)
    with pytest.raises(LD.MmxError):
        LD.normalize([torch.zeros(12000)], 24000, -16.0)


def test_entry_points_are_declared_listed_and_mapped():
    from mmx import _lib
    hdr = open(os.path.join(ROOT, "include", "mmx_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for s in ("mmx_kweight_blocks", "mmx_loudness_gate", "mmx_scale_rows"):
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr) and s in _lib.SYMBOLS and f"`{s}`" in doc and hasattr(lib, s)
    assert int(re.search(r"#define MMX_LOUD_MAX_CH (\d+)", hdr).group(1)) == LD.MAX_CH
    assert {k: int(re.search(r"#define MMX_LOUD_" + k.upper() + r" (\d+)", hdr).group(1)) for k in LD.PARTIAL} == LD.PARTIAL
    assert lib.mmx_abi_version() == 10


@pytest.mark.parametrize("name", ["n7200", "n9600", "n9601", "n12000", "n13001", "tone24k", "zeros", "tone16k", "tone48k"])
def test_fixture_clips_are_decided(name):
    rate, x = fixture_clips()[name]
    for partial in ("pad", "drop"):
        r = reference(name, partial)
        if name == "zeros":
            assert r["lufs"] == -70.0 and not r["keep"].any()
            continue
        l = r["l"][np.isfinite(r["l"])]
        margin = min(np.abs(l + 70.0).min(), np.abs(l - r["gamma_r"]).min())
        assert margin > DECIDED_DB, (name, partial, margin)
        assert r["keep"].any() and r["lufs"] > -70.0
    r = reference(name)
    if name.startswith("tone"):                                 # both gates are at work
        assert (r["l"] <= -70.0).any() and ((r["l"] > -70.0) & (r["l"] <= r["gamma_r"])).any() and r["F"] >= 15
    expect_blocks = {"n7200": 2, "n9600": 2, "n9601": 2, "n12000": 2, "n13001": 3}     # below 0.5 s: padded to 0.5 s = K + S samples
    if name in expect_blocks:
        assert r["F"] == expect_blocks[name]
