"""The sinc resampler on the device (csrc/resample.hip, mmx/resample.py) against the float64 closed form of
tests/test_resample_host.py, then the engine entry points built on it (TtsEngine.prompt_from_clip, reference_embedding(resample=True),
voice_conversion).

Outputs sit in NaN-filled, guarded buffers whose rows are wider than the columns the call may write; input columns at or beyond a
clip's length hold NaN, so a finite result proves nothing beyond `lens` was read.  The per-sample bound is the standard one for
fp32 taps and an fp32 sum of `live` terms, (live + 2) * 2^-24 * sum|h x|; no measured number enters it."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_resample_host as R
import test_s3tok_host as S3

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
PAIRS = R.PAIRS


def bits(t):
    return t.contiguous().view(torch.int32)


def len_for(J, o, n):
    """The longest clip with at most J outputs (at least one sample): exactly J when downsampling, where every count is reached."""
    return max(1, (J * o) // n)


def uniform(L, seed):
    return torch.rand(L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).mul(2).sub(1).float()


_tables = {}


def tables(pair):
    from mmx.resample import _packed
    if pair not in _tables:
        taps, first, count, width = _packed(*pair)
        _tables[pair] = (torch.from_numpy(taps).cuda(), torch.from_numpy(first).cuda(), torch.from_numpy(count).cuda(), width)
    return _tables[pair]


def launch(pair, clips, use_lens=True, tail=3, o_pad=7, w_pad=5):
    """The C entry point on a ragged batch: rows of w_bs = longest + w_pad samples with NaN beyond each clip, an output of
    out_cols = longest output + tail columns in rows of o_bs = out_cols + o_pad, NaN-filled and guarded.  Returns (rc, out [B, o_bs],
    out_cols, per-clip output counts) after checking what must hold for every call: guards and row padding untouched, tails zero."""
    from mmx import _lib as L
    from mmx.resample import out_len
    o, n = R.reduced(*pair)
    taps, first, count, width = tables(pair)
    lens = [int(c.numel()) for c in clips]
    B, Lm = len(clips), max(lens)
    assert use_lens or len(set(lens)) == 1
    wave = torch.full((B, Lm + w_pad), NAN)
    for b, c in enumerate(clips):
        wave[b, :lens[b]] = c
    wave = wave.cuda()
    outs = [out_len(v, *pair) for v in lens]
    cols = max(outs) + tail
    o_bs = cols + o_pad
    buf = torch.full((B * o_bs + 2 * GUARD,), NAN, device="cuda")
    out = buf[GUARD:GUARD + B * o_bs].view(B, o_bs)
    d_lens = torch.tensor(lens, dtype=torch.int32, device="cuda") if use_lens else None
    rc = L.load().mmx_resample_sinc(L._p(wave), L.i64(wave.stride(0)), Lm, B, L._p(d_lens), (C.c_int32 * B)(*lens) if use_lens else None,
                                    o, n, width, L._p(taps), L._p(first), L._p(count), taps.shape[0], L._p(out), L.i64(o_bs), cols,
                                    L.stream())
    torch.cuda.synchronize()
    host = buf.cpu()
    assert torch.isnan(host[:GUARD]).all() and torch.isnan(host[-GUARD:]).all(), "wrote outside its output"
    oh = host[GUARD:GUARD + B * o_bs].view(B, o_bs)
    assert torch.isnan(oh[:, cols:]).all(), "wrote beyond out_cols"
    if rc == 0:
        for b in range(B):
            assert torch.isfinite(oh[b, :outs[b]]).all(), "read at or beyond lens"
            assert (bits(oh[b, outs[b]:cols]) == 0).all(), "tail columns are not zero"
    return rc, oh, cols, outs


def check_against_f64(y, x, pair, what):
    """Every output sample within (live + 2) * 2^-24 * sum|h x| of the closed form on the fp32 input; returns the worst ratio."""
    y64, sabs, live = R.resample_f64(x.numpy(), *pair)
    assert y.shape[0] == y64.shape[0]
    bound = (live + 2) * 2.0 ** -24 * sabs
    err = np.abs(y.double().numpy() - y64)
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
    assert (err <= bound).all(), f"{what}: worst error / bound {ratio:.3f}"
    return ratio, float(bound.max())


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_parity_with_float64_per_sample(pair):
    """Clips whose output counts sit on and around the workgroup's run (1, 2, NOUT - 1, NOUT, NOUT + 1, 3 NOUT + 5; an upsampling pair
    cannot hit every count and takes the next one it has), a clip shorter than the filter's half width and one of 7 samples, all in
    one ragged launch."""
    from mmx.resample import NOUT
    o, n = R.reduced(*pair)
    width = R.width_of(o, n)
    lens = sorted({len_for(J, o, n) for J in (1, 2, NOUT - 1, NOUT, NOUT + 1, 3 * NOUT + 5)} | {max(1, width - 2), 7})
    clips = [uniform(L, 100 + i) for i, L in enumerate(lens)]
    rc, out, _, outs = launch(pair, clips)
    assert rc == 0
    assert {1, 2, NOUT - 1, NOUT, NOUT + 1, 3 * NOUT + 5} <= set(outs) or n > o
    assert max(outs) > 3 * NOUT and min(outs) <= 2
    worst = bmax = 0.0
    for b, x in enumerate(clips):
        r, bm = check_against_f64(out[b, :outs[b]], x, pair, f"{pair} L={lens[b]}")
        worst, bmax = max(worst, r), max(bmax, bm)
    print(f"\n{pair}: lengths {lens} -> outputs {outs}; worst error / bound {worst:.3f}, largest bound {bmax:.2e}")


@pytest.mark.parametrize("pair", [(44100, 16000), (16000, 24000), (48000, 16000)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_ragged_batch_equals_solo_runs_bit_for_bit(pair):
    from mmx.resample import NOUT
    o, n = R.reduced(*pair)
    clips = [uniform(len_for(J, o, n), 7 + i) for i, J in enumerate((3 * NOUT + 5, 1, NOUT))]
    rc, out, _, outs = launch(pair, clips)
    assert rc == 0
    for b, c in enumerate(clips):
        rc1, solo, _, o1 = launch(pair, [c], use_lens=False, tail=0, o_pad=b, w_pad=0)      # lens = NULL: the row is the clip
        assert rc1 == 0 and o1 == [outs[b]]
        assert torch.equal(bits(out[b, :outs[b]]), bits(solo[0, :outs[b]])), f"clip {b} differs from its solo run"
    order = [2, 0, 1]
    rc2, out2, _, outs2 = launch(pair, [clips[i] for i in order], tail=11, o_pad=2, w_pad=9)
    assert rc2 == 0
    for r, b in enumerate(order):
        assert outs2[r] == outs[b] and torch.equal(bits(out2[r, :outs[b]]), bits(out[b, :outs[b]])), f"clip {b} depends on its row"


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_tone_comes_out_at_the_new_rate(pair):
    """A 1 kHz sine of 4000 samples equals the analytic sine at the new rate to 1e-3 away from 200 edge samples (the closed form
    gives <= 5.6e-4 there: the filter's passband ripple)."""
    from mmx.resample import Resample
    orig, new = pair
    x = torch.sin(2 * np.pi * 1000.0 * torch.arange(4000, dtype=torch.float64) / orig).float()
    y = Resample(orig, new)(x.cuda()).cpu().double()
    assert y.shape[0] == -((-4000 * new) // orig)
    want = torch.sin(2 * np.pi * 1000.0 * torch.arange(y.shape[0], dtype=torch.float64) / new)
    err = float((y - want)[200:-200].abs().max())
    e64 = float(np.abs(R.resample_f64(x.numpy(), orig, new)[0] - want.numpy())[200:-200].max())
    print(f"\n{pair}: tone error {err:.2e} (closed form {e64:.2e})")
    assert err <= 1e-3


def test_two_second_clip_48k_to_16k():
    from mmx.resample import Resample, resample
    x = uniform(96000, 3)
    y = Resample(48000, 16000)(x.cuda())
    assert tuple(y.shape) == (32000,) and y.dtype == torch.float32
    ratio, bmax = check_against_f64(y.cpu(), x, (48000, 16000), "2 s clip")
    print(f"\n2 s at 48 kHz -> 16 kHz: worst error / bound {ratio:.3f}, largest bound {bmax:.2e}")
    # the ragged list form and the [B, L] form return the same bits
    short = uniform(5001, 4)
    a, b = resample([x.cuda(), short.cuda().reshape(1, -1)], 48000, 16000)
    assert tuple(a.shape) == (32000,) and tuple(b.shape) == (1667,)
    assert torch.equal(bits(a), bits(y)) and torch.equal(bits(b), bits(Resample(48000, 16000)(short.cuda())))
    two = Resample(48000, 16000)(torch.stack([x, x.flip(0)]).cuda())
    assert tuple(two.shape) == (2, 32000) and torch.equal(bits(two[0]), bits(y))


def test_a_rate_pair_beyond_the_lds_layout_is_refused():
    """16001 -> 16000: 16000 phases of 13 taps are 832 KB of packed bank.  The entry point returns -1 with the output untouched and
    the host raises."""
    from mmx._lib import MmxError
    from mmx.resample import Resample
    x = uniform(4000, 5)
    rc, out, cols, _ = launch((16001, 16000), [x])
    assert rc == -1 and torch.isnan(out).all()
    with pytest.raises(MmxError):
        Resample(16001, 16000)(x.cuda())
    from mmx import _lib as L
    xd = x.cuda()
    for bad in ((2, 2), (4, 2)):                                        # equal / not coprime: the caller reduces the rates
        taps, first, count, width = tables((16000, 24000))
        o = torch.full((64,), NAN, device="cuda")
        rc = L.load().mmx_resample_sinc(L._p(xd), L.i64(4000), 4000, 1, None, None, bad[0], bad[1], width, L._p(taps), L._p(first),
                                        L._p(count), taps.shape[0], L._p(o), L.i64(64), 64, L.stream())
        torch.cuda.synchronize()
        assert rc == -1 and torch.isnan(o).all()


# ------------------------------------------------------------------------------------------------ engine entry points
def _speech(n, rate, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    env = 0.6 + 0.4 * torch.sin(2 * np.pi * 2.5 * t / rate)
    return (0.4 * torch.sin(2 * np.pi * 180.0 * t / rate) * env).float() + 0.05 * torch.randn(n, generator=g)


@pytest.fixture(scope="module")
def eng(golden_dir):
    """As test_prompt_from_audio_splats_into_tts: 2-layer LM, 1 mid block, synthetic DAC, the S3 fixture state, split build."""
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


def test_prompt_from_clip(eng, monkeypatch):
    from mmx.resample import Resample
    calls = []
    run = Resample._run
    monkeypatch.setattr(Resample, "_run", lambda self, w, lens: (calls.append((self.orig_freq, self.new_freq)), run(self, w, lens))[1])
    clip = _speech(57330, 44100, 3).cuda()                               # 1.3 s at 44.1 kHz
    ptext = torch.randint(0, 151936, (1, 4), generator=torch.Generator().manual_seed(1)).cuda()
    r16 = Resample(44100, 16000)(clip)
    assert tuple(r16.shape) == (20800,)
    want = eng.prompt_from_audio(r16, Resample(16000, 24000)(r16), ptext, generator=_gen())
    calls.clear()
    got = eng.prompt_from_clip(clip, 44100, ptext, generator=_gen())
    assert calls == [(44100, 16000), (16000, 24000)]
    _same(got, want)
    assert set(got) == {"llm_prompt_speech_token", "flow_prompt_speech_token", "prompt_speech_feat", "prompt_text", "flow_embedding"}
    direct = eng.prompt_from_audio(r16, Resample(44100, 24000)(clip), ptext, generator=_gen())
    calls.clear()
    _same(eng.prompt_from_clip(clip.reshape(1, -1), 44100, ptext, generator=_gen(), via_16k=False), direct)
    assert calls == [(44100, 16000), (44100, 24000)]
    assert not torch.equal(direct["prompt_speech_feat"], want["prompt_speech_feat"])        # the two routes are different filters
    calls.clear()
    _same(eng.prompt_from_clip(r16, 16000, ptext, generator=_gen()), want)
    assert calls == [(16000, 24000)]                                     # a clip that is at 16 kHz already: one resampling
    text = torch.randint(0, 151936, (1, 8), generator=torch.Generator().manual_seed(0)).cuda()
    wav = eng.tts(text, seed=0, exact_steps=12, **got)
    assert wav.shape[-1] == 24 * eng.hop and torch.isfinite(wav).all()


def test_reference_embedding_resamples_on_request(eng):
    from mmx.resample import Resample
    clip = _speech(62400, 48000, 6).cuda()                               # 1.3 s at 48 kHz
    a = eng.reference_embedding(clip, 48000, resample=True)
    b = eng.reference_embedding(Resample(48000, 24000)(clip), 24000)
    assert tuple(a.shape) == (1, 192) and torch.equal(bits(a), bits(b))
    plain = eng.reference_embedding(clip, 48000)
    assert torch.equal(bits(eng.reference_embedding(clip, 48000, resample=False)), bits(plain))
    assert not torch.equal(a, plain)
    c24 = clip[:31200]
    assert torch.equal(bits(eng.reference_embedding(c24, 24000, resample=True)), bits(eng.reference_embedding(c24, 24000)))


def test_voice_conversion(eng):
    from mmx.resample import Resample
    prompt = eng.prompt_from_clip(_speech(57330, 44100, 3).cuda(), 44100,
                                  torch.randint(0, 151936, (1, 4), generator=torch.Generator().manual_seed(1)).cuda(), generator=_gen())
    src = _speech(28665, 22050, 8).cuda()                                # 1.3 s at 22.05 kHz
    wav = eng.voice_conversion(src, 22050, **prompt).clone()
    tok = eng.s3tok.tokenize([Resample(22050, 16000)(src)])[0].long().reshape(1, -1)
    assert tok.shape[1] == 33
    want = eng.token2wav(tok, prompt["flow_prompt_speech_token"], prompt["prompt_speech_feat"], prompt["flow_embedding"])
    assert tuple(wav.shape) == (1, 1, 2 * tok.shape[1] * eng.hop) and torch.isfinite(wav).all()
    assert torch.equal(bits(wav), bits(want))
    slow = eng.voice_conversion(src, 22050, speed=0.5, **prompt)
    assert tuple(slow.shape) == (1, 1, 4 * tok.shape[1] * eng.hop) and torch.isfinite(slow).all()
