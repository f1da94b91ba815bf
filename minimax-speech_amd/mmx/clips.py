"""The one intake of the audio modules (mel, resample, loudness, metrics, denoise, stoi, degrade; spk and s3tok for pack alone):
what a wrapper does between the caller's clips and the ctypes call, and between the output buffer and the caller's result.  Plain
functions on tensors of any device, so the rules - which ranks are taken, when a copy is made, what `lens` may be - are tested
without a GPU (tests/test_clips_host.py).  `what` is the caller's name: every refusal carries it.  A module's own reasons (minimum
lengths, tap limits, rates) stay in that module's refusal()."""
import ctypes as C

import torch

from ._lib import MmxError, i64


def on_device(what, *tensors):
    """MmxError in the caller's name unless every tensor given (a list is looked through; anything else, None or a span of ints,
    passes) lies in device memory.  A public entry calls this before any other work."""
    for t in tensors:
        for w in (t if isinstance(t, (list, tuple)) else [t]):
            if isinstance(w, torch.Tensor) and not w.is_cuda:
                raise MmxError(f"{what} works on device memory only (no CPU fallback)")


def pack(clips, lens, what):
    """A list of mono clips ([n] / [1, n]), one clip [n], or a padded batch [B, L] / [B, 1, L] with `lens` (a list or a tensor;
    None: every row whole) -> (fp32 [B, L] with unit stride along L, the clips' own lengths as a list of B ints).  One clip stays a
    view where it is fp32 with unit stride already; a [B, L] view into longer rows keeps its row stride; any other stride along L
    forces a copy; a list of several clips is copied into one zero-filled batch.  ValueError for more than one channel, an empty
    list, a wrong number of lengths or a length outside [0, L]."""
    if isinstance(clips, torch.Tensor):
        x = clips[None] if clips.dim() == 1 else clips[:, 0] if clips.dim() == 3 and clips.shape[1] == 1 else clips
        if x.dim() != 2:
            raise ValueError(f"{what}: mono clips only ([n], [B, L] or [B, 1, L]), got {tuple(clips.shape)}")
        x = x.to(torch.float32)
        B, L = x.shape
        if lens is None:
            lens = [L] * B
        else:
            lens = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
            if len(lens) != B:
                raise ValueError(f"{what}: {len(lens)} lengths for {B} clips")
            if not all(0 <= v <= L for v in lens):
                raise ValueError(f"{what}: lengths {lens} are not all within [0, {L}]")
        return (x if x.stride(1) == 1 else x.contiguous()), lens
    ws = list(clips)
    if not ws:
        raise ValueError(f"{what}: no clips")
    if any(w.dim() > 1 and w.numel() != w.shape[-1] for w in ws):
        raise ValueError(f"{what}: mono clips only ([n] or [1, n]), got {[tuple(w.shape) for w in ws]}")
    ws = [w.reshape(-1) for w in ws]
    lens = [int(w.numel()) for w in ws]
    if len(ws) == 1:
        return ws[0].to(torch.float32).contiguous()[None], lens
    x = torch.zeros(len(ws), max(lens), dtype=torch.float32, device=ws[0].device)
    for b, w in enumerate(ws):
        x[b, :lens[b]] = w
    return x, lens


def pack_pair(est, ref, lens, what):
    """pack for an estimate and its reference, two tensors or two lists -> (x, y, lens); ValueError unless clip b of both has one
    length (two tensors: one shape)."""
    if isinstance(est, torch.Tensor) != isinstance(ref, torch.Tensor):
        raise ValueError(f"{what}: estimate and reference come as two tensors or as two lists of clips")
    x, lx = pack(est, lens, what)
    y, ly = pack(ref, lens, what)
    if isinstance(est, torch.Tensor) and x.shape != y.shape:
        raise ValueError(f"{what}: estimate {tuple(est.shape)} and reference {tuple(ref.shape)} differ in shape")
    if lx != ly:
        raise ValueError(f"{what}: estimate and reference clips differ in length: {lx} against {ly}")
    if x.shape[1] < 1:
        raise ValueError(f"{what}: empty clips")
    return x, y, lx


def lens_args(lens, width, dev):
    """(device int32, host c_int32 array) of a list of lengths, or (None, None) where every row has the full width (or `lens` is
    None): an entry point computes the same lengths from NULL as from `width` in every row."""
    if lens is None or all(v == width for v in lens):
        return None, None
    return torch.tensor(lens, dtype=torch.int32, device=dev), (C.c_int32 * len(lens))(*lens)


def row_stride(t):
    """The row stride of [B, L] as i64; one row (whose stride torch leaves arbitrary) counts as L."""
    return i64(t.stride(0) if t.shape[0] > 1 else t.shape[1])


def unpack(out, lens, like):
    """out fp32 [B, L] -> what the caller gets back for `like`, the clips as they were passed: a list of [n] views for a list, a
    tensor of the input's shape ([n], [B, L] or [B, 1, L]) for a tensor."""
    if isinstance(like, torch.Tensor):
        return out.reshape(like.shape)
    return [out[b, :v] for b, v in enumerate(lens)]


def per_clip(v, B, what, none=None):
    """One value or one per clip -> a list of B floats (None entries -> `none`)."""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise ValueError(f"{what}: pass host values (a float or a list), not a device tensor")
        v = v.reshape(-1).tolist()
    vals = list(v) if isinstance(v, (list, tuple)) else [v] * B
    if len(vals) != B:
        raise ValueError(f"{what} is one value or one per clip ({B})")
    return [none if e is None else float(e) for e in vals]


_tables = {}


def device_tables(key, build):
    """What build() returns, held once per key = (module tag, setting .., str(device))."""
    if key not in _tables:
        _tables[key] = build()
    return _tables[key]
