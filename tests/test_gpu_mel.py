"""Reference audio -> speaker embedding on the device: mmx_logmel (csrc/mel.hip) against the float64 golden of
tests/golden/mel.npz (tools/gen_golden_mel.py), its layouts and edge cases, the plumbing up to TtsEngine.tts(reference_audio=),
and LearnableSpeakerEncoder(mean_pooling=True)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SETTING = dict(n_fft=1920, num_mels=80, sampling_rate=24000, hop_size=480, win_size=1920, fmin=0)
LOG_CLIP = float(np.float32(np.log(np.float64(np.float32(1e-5)))))     # fl(ln(fl(1e-5))): log(clamp(v, 1e-5)) of any v <= 1e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mel.npz"))


def _mel(fmax=8000):
    from mmx.mel import LogMel
    return LogMel(fmax=fmax, **SETTING)


@pytest.mark.parametrize("name", ["noise", "tone", "short", "noise_full"])
def test_logmel_parity_with_float64(gold, name):
    """e_gpu = max|logmel_gpu - f64| <= 4 * max(e_ref, 1e-6), e_ref = max|reference fp32 - f64| (the reference runs torch.stft in
    fp32; the kernel a DFT as a GEMM with 24-bit operands and fp32 accumulation over K = 1920).
    Measured on an MI355X, e_gpu / max(e_ref, 1e-6): noise 0.94 (9.4e-7 / 5.1e-7), tone 1.94 (1.17e-4 / 6.0e-5), short 0.66
    (6.6e-7 / 2.9e-7), noise with fmax = None 0.89 (8.9e-7 / 4.6e-7); DESIGN.md §2 has the table."""
    from matcha.utils.audio import mel_spectrogram
    w = torch.from_numpy(gold["wave_" + name.split("_")[0]]).cuda()[None]
    got = mel_spectrogram(w, fmax=None if name.endswith("_full") else 8000, **SETTING)
    r64 = gold[f"ref64_{name}"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + r64.shape
    e_gpu = np.abs(got[0].cpu().numpy().astype(np.float64) - r64).max()
    e_ref = np.abs(gold[f"ref32_{name}"].astype(np.float64) - r64).max()
    print(f"\nlogmel {name}: e_gpu {e_gpu:.3e}  e_ref {e_ref:.3e}  ratio {e_gpu / max(e_ref, 1e-6):.2f}")
    assert e_gpu <= 4 * max(e_ref, 1e-6), (e_gpu, e_ref)


def test_time_major_is_the_transpose_bit_for_bit(gold):
    w = torch.from_numpy(gold["wave_noise"]).cuda()[None]
    m = _mel()
    cm, tm = m(w), m(w, time_major=True)
    assert tuple(cm.shape) == (1, 80, 10) and tuple(tm.shape) == (1, 10, 80)
    assert torch.equal(cm.transpose(1, 2), tm)
    tb = m(w, time_major=True, dtype=1)
    assert tb.dtype == torch.bfloat16 and torch.equal(tb, tm.to(torch.bfloat16))


def test_silence_is_exactly_the_log_of_the_clip():
    y = _mel()(torch.zeros(1, 4800, device="cuda"))
    assert tuple(y.shape) == (1, 80, 10) and bool((y == LOG_CLIP).all()), (y.min().item(), y.max().item(), LOG_CLIP)
    assert abs(LOG_CLIP - math.log(1e-5)) < 1e-6


def test_zero_padded_batch_equals_solo_runs(gold):
    """Lengths (4800, 1440, 2400) in one launch: every member bit-identical to its solo run (its reflection is taken at its own
    end), zeros in the padded frames; the per-member gain is applied in the kernel."""
    m = _mel()
    waves = [torch.from_numpy(gold[k]).cuda() for k in ("wave_noise", "wave_short", "wave_tone")]
    lens = [4800, 1440, 2400]
    batch = torch.zeros(3, 4800, device="cuda")
    for i, w in enumerate(waves):
        batch[i, :lens[i]] = w
    batch[1, 1440:] = 7.0                                    # beyond lens: never read
    gain = torch.tensor([1.0, 0.5, 0.25], device="cuda")
    got = m(batch, lens=lens, gain=gain)
    got_tm = m(batch, lens=lens, gain=gain, time_major=True)
    assert tuple(got.shape) == (3, 80, 10)
    for i, (w, T) in enumerate(zip(waves, (10, 3, 5))):
        solo = m((w * gain[i])[None])
        assert tuple(solo.shape) == (1, 80, T)
        assert torch.equal(got[i, :, :T], solo[0]), i
        assert bool((got[i, :, T:] == 0).all()), i
        assert torch.equal(got_tm[i], got[i].t()), i


def test_a_member_without_reflection_is_refused(gold):
    """720 samples = (n_fft - hop) / 2: the reflection would read sample 720 (torch raises there too) -> MMX_EARG, nothing launched."""
    from mmx._lib import MmxError
    m = _mel()
    with pytest.raises(MmxError, match="code -1"):
        m(torch.zeros(1, 720, device="cuda"))
    batch = torch.zeros(2, 4800, device="cuda")
    with pytest.raises(MmxError, match="code -1"):
        m(batch, lens=[4800, 720])
    assert tuple(m(torch.zeros(1, 721, device="cuda")).shape) == (1, 80, 1)


# ------------------------------------------------------------------------------------------------ plumbing
def _spk_engine(dt):
    from mmx import shapes, synth
    from mmx.spk import SpeakerEncoderEngine
    sd = synth.synth_state_dict(shapes.speaker_encoder_manifest(), 3)
    return SpeakerEncoderEngine(sd, dtype=dt, device="cuda")


def _clip(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    w = 0.3 * torch.sin(2 * math.pi * 220.0 * t / 24000).float() + 0.05 * torch.randn(n, generator=g)
    return w.cuda()


@pytest.mark.parametrize("dt", [0, 2], ids=["fp32", "split"])
def test_embed_audio_equals_the_mel_fed_by_hand(dt):
    from matcha.utils.audio import mel_spectrogram
    from mmx.mel import prepare_reference
    eng = _spk_engine(dt)
    w = _clip(30000)
    seg, gain = prepare_reference(w, 24000)
    assert tuple(seg.shape) == (1, 30000) and abs((seg * gain).abs().max().item() - 1) < 1e-6
    mel = mel_spectrogram(seg * gain, fmax=8000, **SETTING)
    assert tuple(mel.shape) == (1, 80, 62)
    by_hand = eng.reference_embedding(mel)
    got = eng.embed_audio([w])
    assert tuple(got.shape) == (1, 192) and torch.equal(got, by_hand)
    assert abs(got.norm().item() - 1) < 1e-5
    # two clips of one speaker: one zero-padded batch (the collate of processor.py:658; the encoder's attention is unmasked, as
    # in the reference, so the shorter clip's padding frames are attended), the mean of the two embeddings, normalised
    w2 = _clip(18000, seed=6)
    both = eng.embed_audio([w, w2])
    m2 = mel_spectrogram(torch.mul(*prepare_reference(w2, 24000)), fmax=8000, **SETTING)
    assert tuple(m2.shape) == (1, 80, 37)
    e = eng.encode(torch.cat([mel, F.pad(m2, (0, 62 - 37))]))
    assert tuple(both.shape) == (1, 192) and (both - F.normalize(e.mean(0, keepdim=True), dim=1)).abs().max().item() < 1e-6


def test_five_seconds_are_centre_cropped_to_four():
    from mmx.mel import LogMel, prepare_reference
    w = _clip(120000)
    seg, gain = prepare_reference(w, 24000)
    assert tuple(seg.shape) == (1, 96000) and torch.equal(seg[0], w[12000:108000])
    assert torch.equal(gain, 1.0 / w[12000:108000].abs().max().reshape(1))
    assert tuple(_mel()(seg, gain=gain, time_major=True).shape) == (1, 200, 80)
    with pytest.raises(ValueError):
        prepare_reference(w[:11999], 24000)


def test_tts_with_reference_audio_equals_tts_with_its_embedding():
    """TtsEngine.tts(reference_audio=w) == tts(flow_embedding=embed_audio([w])): same tokens, same waveform (the reduced-depth
    configuration of __graft_entry__.smoke with the flow's learnable speaker encoder)."""
    from mmx import shapes, synth
    from mmx.pipeline import TtsEngine
    llm_sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)
    flow_sd = synth.synth_state_dict(shapes.flow_manifest(num_mid_blocks=1, use_speaker_encoder=True), 0)
    dac_sd = synth.synth_state_dict(shapes.dac_decoder_manifest(80), 0)
    text = torch.randint(0, 151936, (1, 8), generator=torch.Generator().manual_seed(0)).cuda()
    w = _clip(36000)
    eng = TtsEngine(llm_sd, flow_sd, dac_sd, dtype=0, max_batch=1, max_ctx=256)
    try:
        e = eng.flow.spk_enc.embed_audio([w])
        a = eng.tts(text, flow_embedding=e, seed=0, exact_steps=12).clone()
        ta = list(eng.llm.tokens()[0])
        b = eng.tts(text, reference_audio=w, seed=0, exact_steps=12).clone()
        assert list(eng.llm.tokens()[0]) == ta and torch.equal(a, b)
        c = eng.tts_batch([text], reference_audio=[w], seed=0, exact_steps=12, overlap=False)[0]
        assert c.shape[-1] == a.shape[-1] and torch.isfinite(c).all()
        with pytest.raises(ValueError):
            eng.tts(text, seed=0, exact_steps=12)
    finally:
        eng.close()
    plain = TtsEngine(llm_sd, {k: v for k, v in flow_sd.items() if not k.startswith("speaker_encoder.")}, dac_sd, dtype=0,
                      max_batch=1, max_ctx=256)
    try:
        with pytest.raises(RuntimeError, match="speaker_encoder"):
            plain.tts(text, reference_audio=w, seed=0, exact_steps=12)
    finally:
        plain.close()


# ------------------------------------------------------------------------------------------------ mean pooling
@pytest.fixture(scope="module")
def spk_case(golden_dir):
    """The weights and mels of spk.npz and, computed once on the CPU from oracle.spk's block stack, the hidden states the pooling reads."""
    import json
    from oracle import spk as OSPK, weights as W
    g = np.load(os.path.join(golden_dir, "spk.npz"))
    man = {k: tuple(v) for k, v in json.load(open(os.path.join(golden_dir, "manifest_spk.json"))).items()}
    sd = W.synth_state_dict(man, 7)
    mels = {37: torch.from_numpy(g["mel_T37"]), 160: F.pad(torch.from_numpy(g["mel_T150"]), (0, 10))}
    hid = {}
    with torch.no_grad():
        for T, mel in mels.items():
            h = F.conv1d(mel, sd["speaker_encoder.init.weight"], sd["speaker_encoder.init.bias"])
            for i in range(6):
                h = OSPK.attention_block(sd, f"speaker_encoder.attn.{i}", h, 8)
            hid[T] = h
    return sd, mels, hid


def _pool_ref(sd, h, mask):
    """llm.py:80-96 on the CPU."""
    if mask is not None:
        pooled = (h * mask).sum(dim=2) / mask.sum(dim=2).clamp(min=1)
    else:
        pooled = h.mean(dim=2)
    return F.normalize(F.linear(pooled, sd["speaker_encoder.output_proj.weight"], sd["speaker_encoder.output_proj.bias"]), p=2, dim=1)


@pytest.mark.parametrize("dt,tol", [(0, 2e-5), (1, 2e-2)], ids=["fp32", "bf16"])
def test_mean_pooling_matches_the_reference_formula(spk_case, dt, tol):
    """Bounds of tests/test_dropin_api.py::test_speaker_encoder_and_flow_with_reference_mels for the same build: the same
    encoder with one reduction added."""
    from cosyvoice.llm.llm import LearnableSpeakerEncoder
    sd, mels, hid = spk_case
    enc = LearnableSpeakerEncoder(mean_pooling=True)
    enc.load_state_dict({k[len("speaker_encoder."):]: v for k, v in sd.items()}, strict=True)
    enc.to("cuda").float_parity(dt == 0)
    mask = torch.zeros(mels[160].shape[0], 1, 160)
    mask[:, :, :150] = 1
    for T, m in ((37, None), (160, None), (160, mask)):
        got = enc(mels[T].cuda(), None if m is None else m.cuda())
        err = (got.cpu() - _pool_ref(sd, hid[T], m)).abs().max().item()
        print(f"\nmean pooling dt {dt} T {T} mask {m is not None}: max err {err:.3e}")
        assert err < tol, (T, m is not None, err)
    first = LearnableSpeakerEncoder()                       # first-frame pooling is what it was
    first.load_state_dict({k[len("speaker_encoder."):]: v for k, v in sd.items()}, strict=True)
    first.to("cuda").float_parity(dt == 0)
    ref0 = F.normalize(F.linear(hid[37][:, :, 0], sd["speaker_encoder.output_proj.weight"], sd["speaker_encoder.output_proj.bias"]), dim=1)
    assert (first(mels[37].cuda()).cpu() - ref0).abs().max().item() < tol
