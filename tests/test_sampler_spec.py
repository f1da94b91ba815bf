"""CPU checks of the per-request sampler plumbing: how Qwen2LM turns its `sampling` callable into a sampler spec for the device
(the three samplers of cosyvoice/utils/common.py, with and without functools.partial keywords; anything else goes to the host),
and the host-side column encoding and range check of the sampler table (include/mmx_hip.h, mmx_sample_step_tab)."""
import struct
from functools import partial

import pytest


def _spec(sampling):
    from cosyvoice.llm.llm import Qwen2LM
    lm = object.__new__(Qwen2LM)                         # the mapping reads `sampling` only: no weights, no GPU
    lm.__dict__["sampling"] = sampling
    return lm._sampler_spec(), lm._is_device_sampler()


def test_reference_samplers_map_to_device_modes():
    from cosyvoice.utils.common import nucleus_sampling, random_sampling, ras_sampling
    assert _spec(ras_sampling) == (dict(mode=0, top_p=0.8, top_k=25, win_size=10, tau_r=0.1), True)
    assert _spec(partial(ras_sampling, top_p=0.7, top_k=12, win_size=20, tau_r=0.3)) == \
        (dict(mode=0, top_p=0.7, top_k=12, win_size=20, tau_r=0.3), True)
    assert _spec(partial(ras_sampling, top_k=5)) == (dict(mode=0, top_p=0.8, top_k=5, win_size=10, tau_r=0.1), True)
    assert _spec(nucleus_sampling) == (dict(mode=1, top_p=0.8, top_k=25), True)
    assert _spec(partial(nucleus_sampling, top_p=0.95, top_k=40)) == (dict(mode=1, top_p=0.95, top_k=40), True)
    assert _spec(random_sampling) == (dict(mode=2), True)
    assert _spec(partial(random_sampling)) == (dict(mode=2), True)


def test_other_callables_go_to_the_host():
    from cosyvoice.utils.common import ras_sampling
    assert _spec(lambda scores, decoded, sampling: scores.argmax()) == (None, False)
    assert _spec(lambda *a, **k: ras_sampling(*a, **k)) == (None, False)         # a wrapper is not the function itself

    def mine(scores, decoded, sampling, top_k=3):
        return scores.argmax()
    assert _spec(partial(mine, top_k=4)) == (None, False)


def test_sampler_column_encoding_and_range_check():
    from mmx import ops
    f32 = lambda v: struct.unpack("<i", struct.pack("<f", v))[0]
    col = ops.sampler_column(mode="random", top_p=0.5, top_k=64, win_size=0, tau_r=2.0, seed=(0x80000001 << 32) | 0xFFFFFFFF)
    assert col == [2, 64, 0, f32(0.5), f32(2.0), -1, -(1 << 31) + 1, 0]
    assert ops.sampler_column() == [0, 25, 10, f32(0.8), f32(0.1), 0, 0, 0]
    assert ops.sampler_column(mode=1, seed=7)[5:7] == [7, 0]
    for bad in (dict(mode=3), dict(mode=-1), dict(mode="greedy"), dict(top_k=0), dict(top_k=65), dict(win_size=-1), dict(win_size=65)):
        with pytest.raises(ValueError):
            ops.sampler_column(**bad)
