"""Host side of the padded attention-map export on the matrix cores (no GPU): the opt-in switch, which entry point _ops.attn_probs
names, and the C-ABI entry point hriemo_attn_probs_mfma."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def maps_switch():
    from hri_emo_amd import _ops
    before = (_ops.MFMA_MAPS, _ops.PACKED_MAPS)
    yield _ops
    _ops.MFMA_MAPS, _ops.PACKED_MAPS = before


def test_the_switch_is_off_by_default_and_exported(maps_switch):
    import hri_emo_amd as H
    _ops = maps_switch
    assert _ops.MFMA_MAPS is False and H.mfma_maps() is False
    assert "set_mfma_maps" in H.__all__ and "mfma_maps" in H.__all__
    H.set_mfma_maps(True)
    assert H.mfma_maps() is True and _ops.MFMA_MAPS is True
    assert _ops.PACKED_MAPS is False          # a switch of its own
    H.set_mfma_maps(0)
    assert H.mfma_maps() is False and _ops.MFMA_MAPS is False
    # a module constant and a setter, not an environment switch
    src = open(os.path.join(REPO, "hri-emo_amd", "_ops.py")).read()
    assert not re.search(r"environ[^\n]*MAPS", src)


def _named(monkeypatch, _ops, cu=None):
    """the entry point _ops.attn_probs hands _lib.call, and its arguments"""
    from hri_emo_amd import _lib
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(_ops, "seed_word", lambda dev: None)
    monkeypatch.setattr(_ops, "_stream", lambda: None)
    B, H, Lq, Lk, hd = 2, 2, 5, 7, 16
    q, k = torch.zeros((B * Lq, H * hd), dtype=torch.bfloat16), torch.zeros((B * Lk, H * hd), dtype=torch.bfloat16)
    kpm = torch.zeros((B, Lk), dtype=torch.uint8)
    lse = torch.zeros((B, H, Lq))
    out = _ops.attn_probs(q, k, B, H, Lq, Lk, hd, None if cu is not None else kpm, lse, 0.0, 0, 0, 0, cu, (Lq, Lk) if cu is not None else None)
    assert out.shape == (B, Lq, Lk) and out.dtype == torch.float32
    assert len(seen) == 1
    return seen[0]


def test_attn_probs_names_the_entry_point_of_the_switch(maps_switch, monkeypatch):
    _ops = maps_switch
    _ops.set_mfma_maps(False)
    name_off, args_off = _named(monkeypatch, _ops)
    assert name_off == "hriemo_attn_probs"
    _ops.set_mfma_maps(True)
    name_on, args_on = _named(monkeypatch, _ops)
    assert name_on == "hriemo_attn_probs_mfma"
    # the same argument list: everything but the three device pointers of the two calls' own tensors
    assert len(args_on) == len(args_off) == 18
    assert args_on[1] == args_off[1] and args_on[3] == args_off[3] and args_on[7:] == args_off[7:]


@pytest.mark.parametrize("on", [False, True])
def test_packed_rows_keep_their_export_whatever_the_switch_says(maps_switch, monkeypatch, on):
    _ops = maps_switch
    _ops.set_mfma_maps(on)
    cu = (torch.tensor([0, 5, 10], dtype=torch.int32), torch.tensor([0, 7, 14], dtype=torch.int32))
    assert _named(monkeypatch, _ops, cu)[0] == "hriemo_attn_probs_varlen"


def test_the_entry_point_is_declared_exported_and_bound():
    from hri_emo_amd import _lib
    hdr = open(os.path.join(REPO, "include", "hriemo.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+hriemo_attn_probs_mfma\s*\(", hdr)
    assert hasattr(L, "hriemo_attn_probs_mfma")
    # the argument list of hriemo_attn_probs
    assert _lib._SIGS["hriemo_attn_probs_mfma"] == _lib._SIGS["hriemo_attn_probs"] == ("plplpppiiiiifQpIip", "i")
    decl = lambda name: re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr).group(1))
    assert decl("hriemo_attn_probs_mfma") == decl("hriemo_attn_probs")
