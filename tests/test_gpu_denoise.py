"""Spectral-gate noise reduction on the device (csrc/denoise.hip mmx_gate_threshold / mmx_gate_analyze / mmx_gate_synthesize,
mmx/denoise.py) against the float64 restatement of tests/test_denoise_host.py, then the engine keyword built on it
(TtsEngine.prompt_from_clip / prompts_from_clips, denoise=).

Shapes: windows 32 / 8 (the smallest: ONE K step of the forward product and two sample tiles, so six of the eight waves idle in the
inverse product and its prefetch runs past the end at once), 128 / 32 (65 bins: the last bin tile is mostly padding; 6 K steps: one
chunk; one sample tile per wave), 512 / 128 (34 K steps: two chunks) and 2048 / 512 (the default: bin 1024 alone in the 65th bin tile,
16 sample tiles per wave, 66 K steps through LDS in four chunks, one of which straddles the real and the imaginary columns).  One
ragged batch per window: 3 frames (n / 2 + 1 samples: every sample under the reflection and the edge envelope), 15 / 16 / 17
frames (a frame-tile boundary under the +-5-frame smoothing and the 4-frame overlap-add) and a long clip; noise clips of 3 frames (the
smallest that exists) and 13.  The batch goes in as a padded tensor whose columns past each clip's length hold NaN: a finite result
proves that nothing past `lens` was read.

Tolerances are 4 x the worst value measured on an MI355X (MEASURED below; the convention of tests/test_gpu_metrics.py), never above
the caps the definitions give: thresholds 0.01 dB; a mask decision may differ from float64's only where |margin| < delta <= 0.05 dB
(test_denoise_host.py holds the share of such bins at or below 1e-3); waveform 2^-16, half a 16-bit PCM step for clips of peak <= 1.
The waveform is checked against the restatement run with the DEVICE's mask, so a legal near-tie flip is not counted as an error."""
import functools

import pytest
import torch

import test_denoise_host as H
import test_s3tok_host as S3

pytestmark = pytest.mark.gpu

CAP_THRESH_DB, CAP_NEAR_DB, CAP_WAVE = 0.01, H.NEAR_DB, 2.0 ** -16
# measured on an MI355X over the batches below: worst |threshold - float64| in dB, the largest |margin64| at a bin whose decision
# differs from float64's (None: no bin differed), worst |waveform - float64 with the device mask|
# (the waveform figure is the larger of the gated batch's and the denoise_amount = 0 round trip's)
MEASURED = {32: (6.154e-6, None, 4.470e-8), 128: (1.059e-4, None, 7.451e-8), 512: (4.862e-4, None, 1.259e-7), 2048: (4.485e-3, None, 1.639e-7)}


def tolerances(n):
    th, flip, wave = MEASURED[n]
    t_th = CAP_THRESH_DB if th is None else min(4 * th, CAP_THRESH_DB)
    t_near = min(4 * (flip if flip is not None else (th if th is not None else CAP_NEAR_DB)), CAP_NEAR_DB)
    return t_th, t_near, CAP_WAVE if wave is None else min(4 * wave, CAP_WAVE)


def bits(t):
    return t.contiguous().view(torch.int32)


def kw(n):
    return dict(win_length=n, hop_length=n // 4)


def padded(xs, extra=7):
    """[B, longest + extra] with NaN past each clip's length, and the lengths."""
    lens = [int(x.numel()) for x in xs]
    t = torch.full((len(xs), max(lens) + extra), float("nan"))
    for b, x in enumerate(xs):
        t[b, :lens[b]] = x
    return t.cuda(), lens


@functools.lru_cache(None)
def device_batch(n):
    """The ragged batch of window n through spectral_gate once: (out [B, L] padded, masks, lens)."""
    from mmx import denoise as D
    xs, nz = H.batch(n)
    x, lens = padded(xs)
    out, masks = D.spectral_gate(x, [z.cuda() for z in nz], lens=lens, return_mask=True, **kw(n))
    torch.cuda.synchronize()
    return out, masks, lens


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("n", H.WINDOWS)
def test_thresholds_against_float64(n):
    """gate_threshold of the 3-frame and the 13-frame noise clip as one ragged batch.  Measured on an MI355X: worst |threshold -
    float64| 6.2e-6 dB at 32, 1.1e-4 dB at 128, 4.9e-4 dB at 512, 4.5e-3 dB at 2048 - there in the 3-frame clip, whose std of three
    values multiplies the dB error of a weak bin (the fp32 restatement's margins are off by up to 1.2e-3 dB on the same fixtures); the
    tolerance is 4 x that, or the 0.01 dB cap where that is lower, as at 2048."""
    from mmx import denoise as D
    nz = H.noise_clips(n)
    got = D.gate_threshold([z.cuda() for z in nz], **kw(n))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, n // 2 + 1)
    want = torch.stack([H.threshold_ref(z, n) for z in nz])
    err = float((got.cpu().double() - want).abs().max())
    print(f"n {n}: worst |threshold - float64| {err:.3e} dB (tolerance {tolerances(n)[0]:.3e})")
    assert err <= tolerances(n)[0]
    for b, z in enumerate(nz):                            # a row is its solo run's, bit for bit
        assert torch.equal(bits(D.gate_threshold(z.cuda(), **kw(n))[0]), bits(got[b]))
    mean = D.gate_threshold(nz[1].cuda(), n_std=0.0, **kw(n))[0].cpu().double()       # n_std = 0: the mean alone
    assert float((mean - H.db(H.stft(nz[1], n)).mean(dim=-1)).abs().max()) <= tolerances(n)[0]


@pytest.mark.parametrize("n", H.WINDOWS)
def test_mask_differs_from_float64_only_at_near_ties(n):
    """Measured on an MI355X: no decision of the 139 908 in the four batches differs from float64's, so delta is 4 x the threshold
    error (2.5e-5 / 4.2e-4 / 1.9e-3 / 1.8e-2 dB), under the 0.05 dB cap."""
    _, masks, lens = device_batch(n)
    delta = tolerances(n)[1]
    worst = 0.0
    for b, (m, (_, margin, m64)) in enumerate(zip(masks, H.batch_ref(n))):
        assert m.dtype == torch.bool and tuple(m.shape) == tuple(m64.shape) == (n // 2 + 1, 1 + lens[b] // (n // 4))
        diff = m.cpu() != m64
        at = float(margin[diff].abs().max()) if diff.any() else 0.0
        worst = max(worst, at)
        print(f"n {n} len {lens[b]}: {int(diff.sum())} of {diff.numel()} decisions differ, largest |margin64| among them {at:.3e} dB")
        assert at < delta, (n, lens[b], at, delta)
    print(f"n {n}: largest |margin64| at a differing bin {worst:.3e} dB (delta {delta:.3e})")


@pytest.mark.parametrize("n", H.WINDOWS)
def test_waveform_against_float64_with_the_device_mask(n):
    """Measured on an MI355X: worst |y - float64| 2.9e-8 at 32, 5.4e-8 at 128, 1.3e-7 at 512, 1.6e-7 at 2048 on clips of peak 0.2 (the
    fp32 restatement: 4.2e-8); the denoise_amount = 0 round trip of test_identities reaches 4.5e-8 / 7.5e-8 / 1.2e-7 / 1.6e-7, and the
    tolerance is 4 x the larger of the two, under the 2^-16 cap."""
    out, masks, lens = device_batch(n)
    xs, nz = H.batch(n)
    tol = tolerances(n)[2]
    assert tuple(out.shape) == (len(xs), max(lens) + 7) and out.dtype == torch.float32
    worst = 0.0
    for b, (x, z) in enumerate(zip(xs, nz)):
        want, _, _ = H.gate_ref(x, z, n, force_mask=masks[b].cpu())
        got = out[b, :lens[b]].cpu()
        assert torch.isfinite(got).all()
        worst = max(worst, float((got.double() - want).abs().max()))
        assert not out[b, lens[b]:].any(), "samples past a member's length are exactly 0"
    print(f"n {n}: worst |waveform - float64 with the device mask| {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol
    # the gate does on the device what it does in float64: the long clip's own lead-in as the noise
    from mmx import denoise as D
    x = H.lead_clip(n)
    lead = x.numel() // 4
    y = D.spectral_gate([x.cuda()], (0, lead), **kw(n))[0].cpu()
    assert H.rms(y[:lead]) <= H.rms(x[:lead]) / 4


@pytest.mark.parametrize("n", H.WINDOWS)
def test_workspace_padding_is_defined(n):
    """mmx_gate_analyze on prefilled workspaces: padded bins and the frames at or past a member's last carry mask 0."""
    from mmx import clips, denoise as D
    from mmx._lib import check, i64, load, stream, _p
    xs, nz = H.batch(n)
    x, lens = padded(xs)
    B, L = x.shape
    nbp, bins, fcap = D.padded_bins(n), n // 2 + 1, D.frames_of(L, n) + 3
    thresh = D.gate_threshold([z.cuda() for z in nz], **kw(n))
    basis, _, _ = D._device_tables(n, x.device)
    d_lens, h_lens = clips.lens_args(lens, L, x.device)
    spec = torch.full((B, fcap, 2 * nbp), float("nan"), device="cuda")
    mask = torch.full((B, fcap, nbp), 255, dtype=torch.uint8, device="cuda")
    check(load().mmx_gate_analyze(_p(x), i64(x.stride(0)), L, B, _p(d_lens), h_lens, _p(basis), n, _p(thresh), i64(bins), _p(spec), _p(mask),
                                  fcap, stream()), "mmx_gate_analyze")
    assert int(mask.max()) == 1 and not mask[:, :, bins:].any()
    _, masks, _ = device_batch(n)
    for b, v in enumerate(lens):
        T = D.frames_of(v, n)
        assert not mask[b, T:].any() and torch.isfinite(spec[b, :T]).all() and not spec[b, :T, bins:nbp].any() and not spec[b, :T, nbp + bins:].any()
        assert torch.equal(mask[b, :T, :bins].t().bool(), masks[b])


# ------------------------------------------------------------------------------------------------ batch independence, identities
@pytest.mark.parametrize("n", H.WINDOWS)
def test_batch_members_equal_their_solo_runs_bit_for_bit(n):
    from mmx import denoise as D
    out, masks, lens = device_batch(n)
    xs, nz = H.batch(n)
    for b, (x, z) in enumerate(zip(xs, nz)):
        (y,), (m,) = D.spectral_gate([x.cuda()], [z.cuda()], return_mask=True, **kw(n))
        assert torch.equal(bits(y), bits(out[b, :lens[b]])) and torch.equal(m, masks[b]), (n, lens[b])
    x, _ = padded(xs)
    again, masks2 = D.spectral_gate(x, [z.cuda() for z in nz], lens=lens, return_mask=True, **kw(n))
    assert torch.equal(bits(again), bits(out)) and all(torch.equal(a, b) for a, b in zip(masks, masks2))
    # as a list of clips (another row order, no padding tensor): the same bits per clip
    ys = D.spectral_gate([x.cuda() for x in reversed(xs)], [z.cuda() for z in reversed(nz)], **kw(n))
    for b, y in enumerate(reversed(ys)):
        assert torch.equal(bits(y), bits(out[b, :lens[b]]))


@pytest.mark.parametrize("n", H.WINDOWS)
def test_identities(n):
    from mmx import denoise as D
    xs, nz = H.batch(n)
    tol = tolerances(n)[2]
    dev = [x.cuda() for x in xs]
    # denoise_amount = 0: STFT -> inverse STFT alone returns the input
    worst = max(float((y.cpu().double() - x.double()).abs().max()) for x, y in zip(xs, D.spectral_gate(dev, nz[0].cuda(), denoise_amount=0.0, **kw(n))))
    print(f"n {n}: round trip (denoise_amount 0) worst |y - x| {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol
    # one amount per clip
    a, b = dev[1], dev[4]
    pair = D.spectral_gate([a, b], nz[0].cuda(), denoise_amount=[0.0, 1.0], **kw(n))
    assert torch.equal(bits(pair[0]), bits(D.spectral_gate([a], nz[0].cuda(), denoise_amount=0.0, **kw(n))[0]))
    assert torch.equal(bits(pair[1]), bits(D.spectral_gate([b], nz[0].cuda(), denoise_amount=1.0, **kw(n))[0]))
    assert not torch.equal(pair[1], b)
    # a shared noise clip equals the same clip passed per member
    shared = D.spectral_gate(dev, nz[0].cuda(), **kw(n))
    each = D.spectral_gate(dev, [nz[0].cuda()] * len(dev), **kw(n))
    assert all(torch.equal(bits(s), bits(e)) for s, e in zip(shared, each))
    # noise=(0, lead) equals passing x[:lead]; the module is the function
    x = H.lead_clip(n).cuda()
    lead = x.numel() // 4
    span = D.spectral_gate([x], (0, lead), **kw(n))[0]
    assert torch.equal(bits(span), bits(D.spectral_gate([x], x[:lead], **kw(n))[0]))
    assert torch.equal(bits(D.SpectralGate()(x[None, None], (0, lead), **kw(n))[0, 0]), bits(span))
    # a half-strength gate lies between the input and the full gate
    half = D.spectral_gate([x], (0, lead), denoise_amount=0.5, **kw(n))[0]
    assert H.rms(span[:lead].cpu()) < H.rms(half[:lead].cpu()) < H.rms(x[:lead].cpu())


def test_refusals_launch_nothing(monkeypatch):
    from mmx import denoise as D
    x = H.clip(24000, 7).cuda()
    monkeypatch.setattr(D, "call", lambda *a: pytest.fail("a refused call reached the library"))
    monkeypatch.setattr(D, "_device_tables", lambda *a: pytest.fail("a refused call built tables"))
    for bad in (dict(win_length=2048, hop_length=256), dict(win_length=2000, hop_length=500), dict(win_length=4096, hop_length=1024)):
        with pytest.raises(D.MmxError):
            D.spectral_gate([x], (0, 6000), **bad)
        with pytest.raises(D.MmxError):
            D.gate_threshold(x[:6000], **bad)
    with pytest.raises(D.MmxError, match="reflected"):    # a clip of n / 2 samples
        D.spectral_gate([x[:1024]], x[:6000])
    with pytest.raises(D.MmxError, match="reflected"):    # a noise clip of n / 2 samples, as a clip and as a span
        D.spectral_gate([x], x[:1024])
    with pytest.raises(D.MmxError, match="reflected"):
        D.spectral_gate([x], (0, 1024))
    with pytest.raises(D.MmxError, match="span"):
        D.spectral_gate([x, x[:5000]], (0, 6000))
    with pytest.raises(D.MmxError, match="no CPU fallback"):
        D.spectral_gate([x.cpu()], (0, 6000))
    with pytest.raises(D.MmxError, match="no CPU fallback"):
        D.spectral_gate([x], x[:6000].cpu())


def test_entry_points_refuse_before_any_launch():
    """The C entry points' own checks (MMX_EARG = -1) with valid pointers: outputs stay untouched."""
    from mmx import denoise as D
    from mmx._lib import i64, load, stream, _p
    import ctypes as C
    n, L = 128, 1500
    x = H.clip(L, 7).cuda()[None]
    basis, inv, win = D._device_tables(n, x.device)
    nbp, fcap = D.padded_bins(n), D.frames_of(L, n)
    work = torch.zeros(1, 8, nbp, 2, dtype=torch.float64, device="cuda")
    thresh = torch.full((1, 65), 7.0, device="cuda")
    spec = torch.zeros(1, fcap, 2 * nbp, device="cuda")
    mask = torch.full((1, fcap, nbp), 9, dtype=torch.uint8, device="cuda")
    frames = torch.zeros(1, fcap, n, device="cuda")
    out = torch.full((1, L), 5.0, device="cuda")
    amt = torch.ones(1, device="cuda")
    lib = load()
    thr = lambda n_fft, Lx, cap: lib.mmx_gate_threshold(_p(x), i64(L), Lx, 1, None, None, _p(basis), n_fft, C.c_double(3.0), _p(work), cap,
                                                         _p(thresh), i64(65), stream())
    assert thr(48, L, 8) == -1 and thr(4096, L, 8) == -1 and thr(n, 64, 8) == -1 and thr(n, L, 1) == -1      # 47 frames: 2 tiles
    ana = lambda n_fft, cap: lib.mmx_gate_analyze(_p(x), i64(L), L, 1, None, None, _p(basis), n_fft, _p(thresh), i64(65), _p(spec), _p(mask), cap,
                                                   stream())
    assert ana(48, fcap) == -1 and ana(n, fcap - 1) == -1
    syn = lambda n_fft, cap, nf, nt: lib.mmx_gate_synthesize(_p(spec), _p(mask), cap, L, 1, None, None, _p(inv), _p(win), n_fft, nf, nt, _p(amt),
                                                              _p(frames), _p(out), i64(L), stream())
    assert syn(48, fcap, 3, 5) == -1 and syn(n, fcap - 1, 3, 5) == -1 and syn(n, fcap, 16, 5) == -1 and syn(n, fcap, 3, -1) == -1
    torch.cuda.synchronize()
    assert float(thresh.min()) == 7.0 and int(mask.min()) == 9 and float(out.min()) == 5.0


# ------------------------------------------------------------------------------------------------ the engine keyword
@pytest.fixture(scope="module")
def eng(golden_dir):
    """As tests/test_gpu_resample.py: 2-layer LM, 1 mid block, synthetic DAC, the S3 fixture state, split build."""
    from mmx import shapes, synth
    from mmx.pipeline import TtsEngine
    z, _ = S3.load_fixture(golden_dir)
    llm_sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)
    flow_sd = synth.synth_state_dict(shapes.flow_manifest(num_mid_blocks=1, use_speaker_encoder=True), 0)
    dac_sd = synth.synth_state_dict(shapes.dac_decoder_manifest(80), 0)
    enc_sd = synth.synth_state_dict(shapes.dac_encoder_manifest(80), 0)
    e = TtsEngine(llm_sd, flow_sd, dac_sd, dtype=2, max_batch=1, max_ctx=256, s3tok_sd=S3.fixture_state(z, "bf16"), dacenc_sd=enc_sd)
    yield e
    e.close()


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def _gen():
    return torch.Generator(device="cuda").manual_seed(9)


def test_prompt_from_clip_denoise(eng, monkeypatch):
    from mmx import denoise as D
    w = (2.0 * H.clip(31200, 7)).cuda()                   # 1.3 s at 24 kHz, peak 0.4
    lead = w.numel() // 4
    ptext = torch.randint(0, 151936, (1, 4), generator=torch.Generator().manual_seed(1)).cuda()
    plain = eng.prompt_from_clip(w, 24000, ptext, generator=_gen())
    with monkeypatch.context() as mp:                     # None: today's path, nothing of the gate is launched
        mp.setattr(D, "spectral_gate", lambda *a, **k: pytest.fail("denoise=None reached the gate"))
        _same(eng.prompt_from_clip(w, 24000, ptext, generator=_gen(), denoise=None), plain)
    clean = D.spectral_gate([w], (0, lead))[0]
    got = eng.prompt_from_clip(w, 24000, ptext, generator=_gen(), denoise={"noise": (0, lead)})
    _same(got, eng.prompt_from_clip(clean, 24000, ptext, generator=_gen()))
    assert not torch.equal(got["prompt_speech_feat"], plain["prompt_speech_feat"])
    # gate first, then level: the meter hears the cleaned clip
    _same(eng.prompt_from_clip(w, 24000, ptext, generator=_gen(), denoise={"noise": (0, lead)}, normalize_db=-20.0),
          eng.prompt_from_clip(clean, 24000, ptext, generator=_gen(), normalize_db=-20.0))
    # a noise clip and the other keywords travel through the dict
    opts = {"noise": w[:lead].clone(), "denoise_amount": 0.5, "win_length": 512, "hop_length": 128, "n_std": 2.0}
    _same(eng.prompt_from_clip(w, 24000, ptext, generator=_gen(), denoise=opts),
          eng.prompt_from_clip(D.spectral_gate([w], w[:lead], denoise_amount=0.5, win_length=512, hop_length=128, n_std=2.0)[0], 24000, ptext,
                               generator=_gen()))
    with pytest.raises(ValueError, match="noise"):
        eng.prompt_from_clip(w, 24000, ptext, denoise={"denoise_amount": 0.5})


def test_prompts_from_clips_denoise(eng):
    from mmx.resample import Resample
    clips = [(2.0 * H.clip(31200, 7)).cuda(), (2.0 * H.clip(28800, 8)).cuda(), (2.0 * H.clip(36000, 9)).cuda().reshape(1, -1)]
    rates = [24000, 24000, 24000]
    dn = [{"noise": (0, 7800)}, None, {"noise": (0, 9000), "denoise_amount": 0.7}]
    g = torch.Generator().manual_seed(4)
    n24 = [Resample(16000, 24000).out_len(Resample(r, 16000).out_len(c.numel())) for c, r in zip(clips, rates)]
    noises = [torch.randn(80, eng.dacenc.frames(v), generator=g).cuda() for v in n24]
    bulk = eng.prompts_from_clips(clips, rates, noises=noises, denoise=dn, normalize_db=[-20.0, None, -18.0])
    for i, db in enumerate((-20.0, None, -18.0)):
        _same(bulk[i], eng.prompt_from_clip(clips[i], rates[i], noise=noises[i][None], denoise=dn[i], normalize_db=db))
    # one dict for all clips
    one = eng.prompts_from_clips(clips[:2], rates[:2], noises=noises[:2], denoise={"noise": (0, 7000)})
    for i in range(2):
        _same(one[i], eng.prompt_from_clip(clips[i], rates[i], noise=noises[i][None], denoise={"noise": (0, 7000)}))
    with pytest.raises(ValueError):
        eng.prompts_from_clips(clips, rates, denoise=[None])
