"""The intake rules of mmx/clips.py on CPU tensors: which ranks pack takes, when it copies, what `lens` may be, how a result goes
back to the caller's form.  The audio modules hold none of this themselves (tests/test_gpu_clips.py runs them through it on the
device)."""
import ctypes

import pytest
import torch

from mmx import clips as CL
from mmx._lib import MmxError

LENS = [1500, 1031, 700]


def ragged(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in LENS]


def padded(ws):
    x = torch.zeros(len(ws), max(w.numel() for w in ws))
    for b, w in enumerate(ws):
        x[b, :w.numel()] = w
    return x


def test_pack_gives_one_batch_for_every_form():
    ws = ragged()
    want = padded(ws)
    forms = [(ws, None), ([w[None] for w in ws], None), (want, LENS), (want[:, None], LENS), (want, torch.tensor(LENS)),
             (want.double(), LENS)]
    for clips, lens in forms:
        x, got = CL.pack(clips, lens, "test")
        assert x.dtype == torch.float32 and x.stride(1) == 1 and torch.equal(x, want)
        assert got == LENS and all(type(v) is int for v in got)
    x, got = CL.pack(want, None, "test")                  # no lens: every row whole, still a list
    assert got == [1500] * 3 and x.data_ptr() == want.data_ptr()


def test_one_clip_stays_a_view():
    w = ragged()[0]
    for form in (w, [w], [w[None]]):
        x, lens = CL.pack(form, None, "test")
        assert tuple(x.shape) == (1, 1500) and lens == [1500] and x.data_ptr() == w.data_ptr()
    x, _ = CL.pack([w.double()], None, "test")            # another type is a copy, in fp32
    assert x.dtype == torch.float32 and torch.equal(x[0], w)


def test_row_stride_is_kept_and_other_strides_are_copied():
    big = padded(ragged())
    view = big[:, 100:500]
    x, lens = CL.pack(view, None, "test")
    assert x.data_ptr() == view.data_ptr() and x.stride() == (1500, 1) and lens == [400] * 3
    assert CL.row_stride(x).value == 1500
    x, lens = CL.pack(big.t(), None, "test")              # [1500, 3] with stride (1, 1500): made contiguous
    assert x.stride() == (3, 1) and x.data_ptr() != big.data_ptr() and torch.equal(x, big.t()) and lens == [3] * 1500


def test_pack_refusals_name_the_caller():
    x = padded(ragged())
    for clips, lens in ((torch.zeros(3, 2, 100), None), ([torch.zeros(2, 100)], None), ([], None), (x, [1500, 1031]),
                        (x, [1500, 1031, 1501]), (x, [1500, -1, 700]), (torch.zeros(2, 1, 3, 100), None)):
        with pytest.raises(ValueError, match="somebody"):
            CL.pack(clips, lens, "somebody")


def test_pack_pair():
    ws = ragged()
    x = padded(ws)
    with pytest.raises(ValueError, match="somebody"):
        CL.pack_pair(ws, x, None, "somebody")
    with pytest.raises(ValueError, match="differ in length"):
        CL.pack_pair(ws, [ws[0], ws[1], ws[2][:699]], None, "somebody")
    with pytest.raises(ValueError, match="differ in length"):
        CL.pack_pair(ws, ws[:2], None, "somebody")
    with pytest.raises(ValueError, match="differ in shape"):
        CL.pack_pair(x, x[:, :1499], None, "somebody")
    with pytest.raises(ValueError, match="empty"):
        CL.pack_pair(torch.zeros(2, 0), torch.zeros(2, 0), None, "somebody")
    a, b, lens = CL.pack_pair(ws, [2 * w for w in ws], None, "test")
    assert torch.equal(a, x) and torch.equal(b, 2 * x) and lens == LENS
    a, b, lens = CL.pack_pair(x[:, None], 2 * x[:, None], LENS, "test")
    assert torch.equal(a, x) and torch.equal(b, 2 * x) and lens == LENS


def test_lens_args():
    assert CL.lens_args([1500] * 3, 1500, "cpu") == (None, None)
    assert CL.lens_args(None, 1500, "cpu") == (None, None)
    for lens, width in ((LENS, 1500), ([1500] * 3, 1501), ([0, 1500], 1500)):
        d, h = CL.lens_args(lens, width, "cpu")
        assert d.dtype == torch.int32 and d.tolist() == lens and list(h) == lens and h._type_ is ctypes.c_int32


def test_row_stride():
    assert CL.row_stride(torch.zeros(1, 70)).value == 70
    assert CL.row_stride(torch.zeros(100, 70)[40:41]).value == 70        # one row: its stride plays no part
    assert CL.row_stride(torch.zeros(3, 70)).value == 70
    assert CL.row_stride(torch.zeros(3, 70)[:, 10:20]).value == 70


def test_unpack():
    ws = ragged()
    x, lens = CL.pack(ws, None, "test")
    got = CL.unpack(x, lens, ws)
    assert isinstance(got, list) and all(torch.equal(g, w) and g.data_ptr() == x[b].data_ptr() for b, (g, w) in enumerate(zip(got, ws)))
    for like in (ws[0], x, x[:, None]):
        out, _ = CL.pack(like, None, "test")
        assert CL.unpack(out, None, like).shape == like.shape


def test_per_clip():
    assert CL.per_clip(2, 3, "v") == [2.0, 2.0, 2.0]
    assert CL.per_clip([1, None, 3.5], 3, "v", none=-1.0) == [1.0, -1.0, 3.5]
    assert CL.per_clip((1, 2), 2, "v") == [1.0, 2.0]
    assert CL.per_clip(torch.tensor([0.5, 0.25]), 2, "v") == [0.5, 0.25]
    assert CL.per_clip(None, 2, "v") == [None, None]
    for v, B in (([1, 2], 3), (torch.zeros(4), 3), ([], 1)):
        with pytest.raises(ValueError, match="somebody"):
            CL.per_clip(v, B, "somebody")


def test_device_only_refusal():
    x = torch.zeros(4)
    for args in ((x,), ([x, x],), (None, (0, 4), x)):
        with pytest.raises(MmxError, match="somebody works on device memory only \\(no CPU fallback\\)"):
            CL.on_device("somebody", *args)
    CL.on_device("somebody", None, (0, 4), 3.0, [])       # nothing that is a tensor: passes


def test_device_tables_build_once_per_key():
    calls = []
    for _ in range(2):
        assert CL.device_tables(("test_clips_host", 7, "cpu"), lambda: calls.append(1) or "table") == "table"
    assert calls == [1]
