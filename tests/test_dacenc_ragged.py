"""DacEncoderEngine.encode_ragged / fuse_ru and the entry points on top of them: TtsEngine.prompts_from_clips and
batch_prompt_args, DACVAE.encode_batch, latents.latent_records / save_latents.

CPU (not marked gpu): the per-member length chain against DacEncoderEngine.frames and torch's Conv1d floors, and the argument
guards that run without the library.  GPU: a ragged batch gives every member the bits of its own solo encode (fp32 / bf16 / split
builds unfused, bf16 / split fused, and a batch whose lengths straddle the fused tiles' edges at both fused stages); the fused
engine against the reference's recorded outputs; the bulk entry points against their per-clip counterparts."""
import math
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

ENC_RATES = [2, 3, 4, 4, 5]
SEED = 7
X2 = 2
# default tiles of mmx_dac_ru at the encoder's fused stages, C = 64 (24 kHz rows) and C = 128 (12 kHz rows): the static_asserts
# under dac_ru_select in csrc/fused.hip
FUSED_BM = {1: (128, 128), X2: (64, 64)}


def _sd(golden_dir):
    from oracle import weights as W
    return W.synth_state_dict(W.load_manifest(os.path.join(golden_dir, "manifest_dacenc.json")), SEED)


_ENGINES = {}


def _engine(golden_dir, dt, fused=False, device="cuda"):
    from mmx.dac import DacEncoderEngine
    key = (dt, fused, device)
    if key not in _ENGINES:
        _ENGINES[key] = DacEncoderEngine(_sd(golden_dir), ENC_RATES, dtype=dt, device=device, fuse_ru=fused)
    return _ENGINES[key]


def bits(t):
    return t.contiguous().view(torch.int32)


# ================================================================================================ CPU
def test_member_length_chain_matches_frames_and_conv1d_floors(golden_dir):
    eng = _engine(golden_dir, 0, device="cpu")
    assert eng.hop == 480
    convs = [torch.nn.Conv1d(1, 1, 2 * s, stride=s, padding=math.ceil(s / 2)) for s in ENC_RATES]
    for k in (1, 2, 3, 5, 10, 23):
        for off in (-1, 0, 1, 7):
            n = k * 480 + off
            chain = eng.stage_lens(n)
            assert chain[0] == n and len(chain) == len(ENC_RATES) + 1
            x = torch.zeros(1, 1, n)
            for st, conv in enumerate(convs):
                x = conv(x)
                assert chain[st + 1] == x.shape[-1] == eng._down(chain[st], ENC_RATES[st]), (n, st)
            assert chain[-1] == eng.frames(n) >= 1
            if off == 0:
                assert chain[-1] == k


def test_encode_ragged_argument_guards(golden_dir):
    eng = _engine(golden_dir, 0, device="cpu")
    ok = torch.zeros(4800)
    with pytest.raises(ValueError, match="non-empty list"):
        eng.encode_ragged([])
    with pytest.raises(ValueError, match="non-empty list"):
        eng.encode_ragged(ok)
    with pytest.raises(ValueError, match="1 noise tensors for 2 clips"):
        eng.encode_ragged([ok, ok], noises=[torch.zeros(80, 10)])
    with pytest.raises(ValueError, match=r"shorter than one latent frame \(clip 1\)"):
        eng.encode_ragged([ok, torch.zeros(100)])
    with pytest.raises(ValueError, match="clip 0: a mono tensor"):
        eng.encode_ragged([torch.zeros(2, 4800)])
    with pytest.raises(ValueError, match="clip 0 is not on the device"):
        eng.encode_ragged([ok, torch.zeros(1, 960)], noises=[torch.zeros(80, 10), torch.zeros(80, 2)])
    with pytest.raises(ValueError, match=r"noise 0 has shape \(80, 9\)"):
        eng.encode_ragged([ok], noises=[torch.zeros(80, 9)])


def test_fuse_ru_is_off_by_default_and_ignored_by_the_fp32_build(golden_dir):
    from mmx.dac import DacEncoderEngine
    sd = _sd(golden_dir)
    assert not _engine(golden_dir, 0, device="cpu").fuse_ru
    e = DacEncoderEngine(sd, ENC_RATES, dtype=0, device="cpu", fuse_ru=True)
    assert not e.fuse_ru and not any(b["fused"] for b in e.blocks) and [b["c"] for b in e.blocks[:2]] == [64, 128]


def test_batch_prompt_args():
    from mmx.pipeline import TtsEngine
    ps = [{"llm_prompt_speech_token": 1, "flow_prompt_speech_token": 2, "prompt_speech_feat": 3, "prompt_text": 4, "flow_embedding": 5},
          {"llm_prompt_speech_token": 6, "flow_prompt_speech_token": 7, "prompt_speech_feat": 8}]
    assert TtsEngine.batch_prompt_args(ps) == {"prompt_texts": [4, None], "llm_prompt_speech_tokens": [1, 6], "flow_prompt_speech_tokens": [2, 7],
                                               "prompt_speech_feats": [3, 8], "flow_embeddings": [5, None]}
    assert "flow_embeddings" not in TtsEngine.batch_prompt_args(ps[1:])


# ================================================================================================ GPU: ragged = solo
def _clips(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [(0.3 * torch.randn(n, generator=g)).cuda() for n in lens]


def _ragged_equals_solo(eng, lens, seed):
    clips = _clips(lens, seed)
    g = torch.Generator().manual_seed(seed + 1)
    noises = [torch.randn(eng.D, eng.frames(n), generator=g).cuda() for n in lens]
    got = eng.encode_ragged([clips[0].reshape(1, -1)] + clips[1:], noises=noises)
    assert len(got) == len(lens)
    for b, n in enumerate(lens):
        solo = eng.encode(clips[b][None, None], noise=noises[b][None])
        for name, r, s in zip(("z", "mu", "logs"), got[b], solo):
            assert tuple(r.shape) == (eng.D, eng.frames(n)) and bool(torch.isfinite(r).all())
            assert torch.equal(bits(r), bits(s[0])), f"member {b} ({n} samples): {name} differs from its solo encode"


@gpu
@pytest.mark.parametrize("dt,fused", [(0, False), (1, False), (X2, False), (1, True), (X2, True)], ids=["f32", "bf16", "x2", "bf16-fused", "x2-fused"])
def test_encode_ragged_equals_solo_bit_for_bit(golden_dir, dt, fused):
    eng = _engine(golden_dir, dt, fused)
    assert eng.fuse_ru == fused and [b["fused"] for b in eng.blocks] == [fused, fused, False, False, False]
    _ragged_equals_solo(eng, [4800, 4807, 2400 + 13, 960], 11)


@gpu
@pytest.mark.parametrize("dt", [1, X2], ids=["bf16", "x2"])
def test_encode_ragged_lengths_on_the_fused_tile_edges(golden_dir, dt):
    """Members whose ends sit on, one row before and one or two rows behind a tile edge of BOTH fused stages (rows of the second are
    _down(n, 2) = n // 2), inside the halo behind one, and in the batch's last partial tile."""
    eng = _engine(golden_dir, dt, True)
    bm1, bm2 = FUSED_BM[dt]
    L0 = 1024
    assert L0 % bm1 == 0 and eng.stage_lens(L0)[1] % bm2 == 0 and eng.stage_lens(L0 + 2)[1] % bm2 == 1
    _ragged_equals_solo(eng, [L0, L0 + 1, L0 - 1, L0 + 2, L0 + bm1 // 2 + 6, 2 * L0 + 5], 13)


@gpu
def test_encode_ragged_with_a_generator_uses_one_draw(golden_dir):
    eng = _engine(golden_dir, 0)
    lens = [4800, 960]
    clips = _clips(lens, 3)
    gen = lambda: torch.Generator(device="cuda").manual_seed(5)
    got = eng.encode_ragged(clips, generator=gen())
    draw = torch.randn(2, 10, eng.D, device="cuda", generator=gen())
    want = eng.encode_ragged(clips, noises=[draw[b, :eng.frames(n)].t().contiguous() for b, n in enumerate(lens)])
    for g_, w_ in zip(got, want):
        for a, b in zip(g_, w_):
            assert torch.equal(bits(a), bits(b))
    with pytest.raises(ValueError, match="not on the device"):
        eng.encode_ragged([clips[0], clips[1].cpu()])


# ================================================================================================ GPU: fused vs the reference
def _golden_runs(eng, golden_dir):
    """-> {clip: (mu err, logs err, z rel err)} against the reference's recorded outputs: 4800 and 11000 samples padded to the hop
    (DACVAE.preprocess), 11000 raw (clamped, unpadded: extract_dac_latents.py)."""
    from oracle import dac as ODAC
    g = np.load(os.path.join(golden_dir, "dacenc.npz"))
    t = lambda k: torch.from_numpy(g[k])
    runs = [(f"{n}", ODAC.preprocess(t(f"wav_{n}"), 480), f"noise_{n}", f"mu_{n}", f"logs_{n}", f"z_{n}") for n in (4800, 11000)]
    runs.append(("11000 raw", t("wav_11000").clamp(-1.0, 1.0), "noise_raw_11000", "mu_raw_11000", "logs_raw_11000", "z_raw_11000"))
    out = {}
    for name, x, kn, km, kl, kz in runs:
        z, mu, logs = eng.encode(x.cuda(), noise=t(kn).cuda())
        assert mu.shape == t(km).shape
        out[name] = ((mu.cpu() - t(km)).abs().max().item(), (logs.cpu() - t(kl)).abs().max().item(),
                     ((z.cpu() - t(kz)).abs() / (1 + t(kz).abs())).max().item())
    return out


@gpu
def test_fused_bf16_encode_vs_reference_golden(golden_dir):
    """The tolerances test_dac_encode_vs_reference_golden (tests/test_gpu_dac.py) applies to the bf16 build: 8e-2 abs on mu and
    logs, 0.3 on |z - ref| / (1 + |ref|)."""
    for name, (emu, elogs, ez) in _golden_runs(_engine(golden_dir, 1, True), golden_dir).items():
        print(f"fused bf16, clip {name}: mu {emu:.3e} logs {elogs:.3e} z {ez:.3e}")
        assert emu < 8e-2 and elogs < 8e-2 and ez < 0.3, (name, emu, elogs, ez)


@gpu
def test_fused_split_encode_vs_reference_golden(golden_dir):
    """The split build has no recorded tolerance: the fused engine is held to 3 x the error the unfused split engine itself has on
    the same clip against the same recorded outputs."""
    plain = _golden_runs(_engine(golden_dir, X2, False), golden_dir)
    fused = _golden_runs(_engine(golden_dir, X2, True), golden_dir)
    for name in plain:
        print(f"split, clip {name}: unfused mu {plain[name][0]:.3e} logs {plain[name][1]:.3e} z {plain[name][2]:.3e} | "
              f"fused mu {fused[name][0]:.3e} logs {fused[name][1]:.3e} z {fused[name][2]:.3e}")
    for name in plain:
        for what, p, f in zip(("mu", "logs", "z"), plain[name], fused[name]):
            assert f <= 3 * p, (name, what, f, p)


# ================================================================================================ GPU: bulk entry points
def _speech(n, rate, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    env = 0.6 + 0.4 * torch.sin(2 * np.pi * 2.5 * t / rate)
    return (0.4 * torch.sin(2 * np.pi * (150.0 + 20 * seed) * t / rate) * env).float() + 0.05 * torch.randn(n, generator=g)


def _tts_engine(golden_dir, dtype, **kw):
    """2-layer LM, 1 mid block, synthetic DAC, the S3 fixture state, three decode slots."""
    import test_s3tok_host as S3
    from mmx import shapes, synth
    from mmx.pipeline import TtsEngine
    z, _ = S3.load_fixture(golden_dir)
    llm_sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)
    flow_sd = synth.synth_state_dict(shapes.flow_manifest(num_mid_blocks=1, use_speaker_encoder=True), 0)
    dac_sd = synth.synth_state_dict(shapes.dac_decoder_manifest(80), 0)
    enc_sd = synth.synth_state_dict(shapes.dac_encoder_manifest(80), 0)
    return TtsEngine(llm_sd, flow_sd, dac_sd, dtype=dtype, max_batch=3, max_ctx=256, s3tok_sd=S3.fixture_state(z, "bf16"), dacenc_sd=enc_sd, **kw)


@pytest.fixture(scope="module")
def tts(golden_dir):
    e = _tts_engine(golden_dir, 2)
    yield e
    e.close()


@gpu
def test_dacenc_fused_flag_reaches_the_encoder(golden_dir):
    """TtsEngine(dacenc_fused=True), bf16 build: the prompt encoder runs its first two stages fused, and the bulk prompts equal the
    per-clip ones of the same engine."""
    eng = _tts_engine(golden_dir, 1, dacenc_fused=True)
    try:
        assert eng.dacenc.fuse_ru and [b["fused"] for b in eng.dacenc.blocks[:3]] == [True, True, False]
        clips, rates = [_speech(24000, 24000, 1).cuda(), _speech(35000, 44100, 2).cuda()], [24000, 44100]
        bulk = eng.prompts_from_clips(clips, rates, generator=torch.Generator(device="cuda").manual_seed(1))
        n1 = bulk[1]["prompt_speech_feat"].shape[1]
        assert "prompt_text" not in bulk[0] and n1 > 0 and n1 % 2 == 0
        g = torch.Generator().manual_seed(2)
        noises = [torch.randn(80, eng.dacenc.frames(RS_len(r, c.numel())), generator=g).cuda() for c, r in zip(clips, rates)]
        bulk = eng.prompts_from_clips(clips, rates, noises=noises)
        for i in range(2):
            solo = eng.prompt_from_clip(clips[i], rates[i], noise=noises[i][None])
            assert set(bulk[i]) == set(solo) and all(torch.equal(bulk[i][k], solo[k]) for k in solo), i
    finally:
        eng.close()


def RS_len(rate, n):
    """Samples of a clip of n samples at `rate` after prompt_from_clip's route to 24 kHz (via 16 kHz)."""
    from mmx.resample import Resample
    return Resample(16000, 24000).out_len(Resample(rate, 16000).out_len(n))


@gpu
def test_prompts_from_clips_equal_prompt_from_clip(tts, monkeypatch):
    from mmx import resample as RS
    from mmx.s3tok import SpeechTokenizerEngine
    eng = tts
    assert eng.dacenc_fused is False and not eng.dacenc.fuse_ru
    clips = [_speech(44100, 44100, 1).cuda(), _speech(48000, 48000, 2).cuda(), _speech(57330, 44100, 3).cuda().reshape(1, -1)]
    rates = [44100, 48000, 44100]
    g = torch.Generator().manual_seed(4)
    ptexts = [torch.randint(0, 151936, (1, 3 + i), generator=g).cuda() for i in range(3)]
    n24 = [RS.Resample(16000, 24000).out_len(RS.Resample(r, 16000).out_len(c.numel())) for c, r in zip(clips, rates)]
    noises = [torch.randn(80, eng.dacenc.frames(n), generator=g).cuda() for n in n24]
    solo = [eng.prompt_from_clip(c, r, t, noise=nz[None]) for c, r, t, nz in zip(clips, rates, ptexts, noises)]
    calls = {"resample": [], "tokenize": 0, "encode_ragged": 0}
    run, tok, enc = RS.Resample._run, SpeechTokenizerEngine.tokenize, type(eng.dacenc).encode_ragged
    monkeypatch.setattr(RS.Resample, "_run", lambda self, w, lens: (calls["resample"].append((self.orig_freq, self.new_freq, w.shape[0])), run(self, w, lens))[1])
    monkeypatch.setattr(SpeechTokenizerEngine, "tokenize", lambda self, w: (calls.__setitem__("tokenize", calls["tokenize"] + 1), tok(self, w))[1])
    monkeypatch.setattr(type(eng.dacenc), "encode_ragged", lambda self, *a, **k: (calls.__setitem__("encode_ragged", calls["encode_ragged"] + 1), enc(self, *a, **k))[1])
    bulk = eng.prompts_from_clips(clips, rates, ptexts, noises=noises)
    monkeypatch.undo()
    # the clips that share a rate: one launch; one tokenizer batch, one encode
    assert sorted(calls["resample"]) == [(16000, 24000, 3), (44100, 16000, 2), (48000, 16000, 1)]
    assert calls["tokenize"] == 1 and calls["encode_ragged"] == 1
    assert len(bulk) == 3
    for i in range(3):
        assert set(bulk[i]) == set(solo[i]) == {"llm_prompt_speech_token", "flow_prompt_speech_token", "prompt_speech_feat", "prompt_text", "flow_embedding"}
        for k in solo[i]:
            a, b = bulk[i][k], solo[i][k]
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (i, k)
    direct = eng.prompts_from_clips(clips, rates, ptexts, noises=noises, via_16k=False)
    want = eng.prompt_from_clip(clips[1], 48000, ptexts[1], noise=noises[1][None], via_16k=False)
    assert all(torch.equal(direct[1][k], want[k]) for k in want)
    with pytest.raises(ValueError, match="per clip"):
        eng.prompts_from_clips(clips, rates[:2])
    texts = [torch.randint(0, 151936, (1, 6 + i), generator=g).cuda() for i in range(3)]
    kw = eng.batch_prompt_args(bulk)
    assert set(kw) == {"prompt_texts", "llm_prompt_speech_tokens", "flow_prompt_speech_tokens", "prompt_speech_feats", "flow_embeddings"}
    wavs = eng.tts_batch(texts, seed=2, exact_steps=[10, 12, 14], overlap=False, **kw)
    ids = [t.clone() for t in eng.last_tokens]
    assert len(wavs) == 3 and all(bool(torch.isfinite(w).all()) for w in wavs) and [t.numel() for t in ids] == [10, 12, 14]
    eng.tts_batch(texts, seed=2, exact_steps=[10, 12, 14], overlap=False, **eng.batch_prompt_args(solo))
    for i in range(3):
        assert torch.equal(ids[i], eng.last_tokens[i]), i


@gpu
def test_latent_records_and_save_latents(golden_dir, tmp_path):
    import latents
    from oracle import weights as W
    from test_dropin_api import _ref, build_dac
    dac = build_dac(80)
    dac.load_state_dict(W.synth_state_dict({**_ref(golden_dir, "dac80"), **_ref(golden_dir, "dacenc")}, 7), strict=True)
    dac.to("cuda").float_parity()
    g = torch.Generator().manual_seed(21)
    wavs = [(1.2 * torch.rand(n, generator=g) - 0.6) * 2.2 for n in (11000, 4800, 5283)]          # some samples beyond [-1, 1]: the clamp
    paths = [str(tmp_path / "spk1" / f"utt{i}.wav") for i in range(3)]
    recs = latents.latent_records(dac, [wavs[0].numpy(), wavs[1], wavs[2]], 24000, paths)
    for i, (w, rec) in enumerate(zip(wavs, recs)):
        one = latents.latent_record(dac, w, 24000, paths[i])
        assert set(rec) == set(one)
        for k in one:
            if k in ("mu", "logs"):
                assert rec[k].shape == one[k].shape and torch.equal(bits(rec[k]), bits(one[k])), (i, k)
            elif k == "z":                                              # another draw: same shape, same distribution parameters
                assert rec[k].shape == one[k].shape and bool(torch.isfinite(rec[k]).all())
            else:
                assert rec[k] == one[k], (i, k)
    # z itself: with the draw given, a member's z is its solo z
    nz = [torch.randn(80, r["latent_shape"][1], generator=g).cuda() for r in recs]
    batch = dac.encode_batch([torch.clamp(w.cuda(), -1.0, 1.0).reshape(1, 1, -1) for w in wavs[:2]] + [torch.clamp(wavs[2].cuda(), -1.0, 1.0)], noises=nz)
    assert batch[0][0].dim() == 3 and batch[2][0].dim() == 2
    for i, w in enumerate(wavs):
        z, m, logs = dac.encode(torch.clamp(w.cuda(), -1.0, 1.0).reshape(1, 1, -1), noise=nz[i][None])
        for a, b in zip(batch[i], (z, m, logs)):
            assert torch.equal(bits(a.reshape(b.shape[1:])), bits(b[0])), i
        assert torch.equal(bits(batch[i][1].reshape(80, -1).cpu()), bits(recs[i]["mu"]))
    outs = latents.save_latents(dac, wavs, 24000, paths)
    assert [os.path.basename(o) for o in outs] == [f"utt{i}_latent2x.pt" for i in range(3)]
    for i, o in enumerate(outs):
        rec = torch.load(o, map_location="cpu", weights_only=False)
        assert rec["original_samples"] == wavs[i].numel() and rec["original_path"] == paths[i] and torch.equal(rec["mu"], recs[i]["mu"])
        lat, tok = latents.load_speech_latent(o, list(range(4)), 2)
        assert lat.shape == (8, 80) and len(tok) == 4 and torch.equal(lat, rec["z"].t()[:8])
    with pytest.raises(ValueError, match="resampled"):
        latents.latent_records(dac, wavs, 16000)
    with pytest.raises(ValueError, match="paths for"):
        latents.latent_records(dac, wavs, 24000, paths[:1])
