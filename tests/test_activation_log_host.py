"""CPU suite of the activation log (hri_emo_amd.train.ActivationLog, csrc/actlog.hip): the decode of hand-written ring images
(wrap-around, closed passes, an absent half), the blame rule, the site table the log builds from a model, the sites= patterns and
the refusals, the three ABI entries in header, library and binding, and the float64 reference of actlog_reference.py against
hand-counted cases."""
import numpy as np
import pytest
import torch

import actlog_reference as R

NAMES_1 = ["input.audio", "input.text", "enc0.audio_self", "enc0.text_self", "enc0.audio_cross", "enc0.audio_ffn", "enc0.text_cross",
           "enc0.text_ffn", "gate.w", "gate.fused", "dec0.self", "dec0.cross", "dec0.ffn", "logits"]


def _model(layers, d=64):
    from hri_emo_amd import FusionWithEmotionDecoder
    torch.manual_seed(0)
    return FusionWithEmotionDecoder(d_model=d, num_emotions=4, n_heads=2, num_layers_fusion=layers, num_layers_decoder=layers,
                                    beta_hidden=32, dropout=0.1)


def _image(names, capacity, records, n_passes):
    """a host image of the log's state after `records` = [(pass, halves, {(half, site): (n_rows, n_bad, first, absmax, sumsq)})] were
    written in order into a ring of `capacity` slots"""
    from hri_emo_amd.train import ActivationLog as L
    S = len(names)
    ring_at = L.HEADER + (2 * S + 3) // 4 * 4
    rw = L.REC_HEADER + 2 * S * L.ENTRY
    img = np.zeros(ring_at + capacity * rw, dtype=np.int32)
    img[0], img[1] = n_passes, len(records)
    for r, (p, halves, entries) in enumerate(records):
        rec = img[ring_at + (r % capacity) * rw:][:rw]
        rec[:] = 0
        rec[0], rec[1] = p, halves
        for (half, site), (n_rows, n_bad, first, absmax, sumsq) in entries.items():
            e = rec[L.REC_HEADER + (half * S + site) * L.ENTRY:][:L.ENTRY]
            e[:4] = (1, n_rows, n_bad, first)
            e[4:6] = np.array([absmax, sumsq], dtype=np.float32).view(np.int32)
    return img


# ------------------------------------------------------------------------------------------------------------ decode
def test_decode_reads_records_oldest_first_and_forms_rms_in_float64():
    from hri_emo_amd.train import ActivationLog as L
    names, widths = ["a", "b", "c"], [8, 8, 4]
    recs = [(0, 3, {(0, 0): (10, 0, -1, 2.0, 40.0), (0, 1): (5, 0, -1, 1.0, 10.0), (1, 0): (10, 0, -1, 0.5, 5.0)}),
            (3, 1, {(0, 0): (10, 2, 7, 3.0, 80.0), (0, 2): (6, 0, -1, 4.0, 24.0)})]
    arr = L.decode(_image(names, 4, recs, n_passes=5), names, widths, 4)
    assert arr["sites"] == names and arr["n_passes"] == 5 and arr["n_recorded"] == 2      # passes 1, 2, 4 ran closed: no record
    assert arr["pass"].tolist() == [0, 3] and arr["halves"].tolist() == [3, 1]
    f, g = arr["forward"], arr["gradient"]
    assert f["have"].tolist() == [[1, 1, 0], [1, 0, 1]] and g["have"].tolist() == [[1, 0, 0], [0, 0, 0]]      # a half with have = 0
    assert f["n_bad"][1].tolist() == [2, 0, 0] and f["first_bad_row"][1, 0] == 7
    assert f["absmax"].dtype == np.float32 and f["absmax"][1, 2] == 4.0 and f["sumsq"][0, 0] == 40.0
    assert f["rms"].dtype == np.float64
    assert f["rms"][0, 0] == np.sqrt(40.0 / (10 * 8)) and f["rms"][1, 2] == np.sqrt(24.0 / (6 * 4))
    assert np.isnan(f["rms"][0, 2]) and np.isnan(g["rms"][1, 0])


def test_decode_unwraps_a_ring_that_wrapped():
    from hri_emo_amd.train import ActivationLog as L
    names, widths = ["a", "b"], [8, 8]
    recs = [(p, 1, {(0, 0): (p + 1, 0, -1, float(p), float(p))}) for p in range(7)]
    arr = L.decode(_image(names, 3, recs, n_passes=7), names, widths, 3)
    assert arr["n_recorded"] == 7 and arr["pass"].tolist() == [4, 5, 6]
    assert arr["forward"]["n_rows"][:, 0].tolist() == [5, 6, 7]
    empty = L.decode(_image(names, 3, [], n_passes=0), names, widths, 3)
    assert len(empty["pass"]) == 0 and L.blame_of(empty, [1, 1]) is None
    with pytest.raises(ValueError, match="image"):
        L.decode(np.zeros(7, np.int32), names, widths, 3)


# ------------------------------------------------------------------------------------------------------------ blame
def test_blame_rule():
    from hri_emo_amd.train import ActivationLog as L
    names, widths, row_len = ["a", "b", "c", "d"], [8] * 4, [20, 12, 4, 1]
    clean = {(h, s): (10, 0, -1, 1.0, 1.0) for h in (0, 1) for s in range(4)}

    def blame(entries, record=-1, extra=()):
        recs = list(extra) + [(0, 3, entries)]
        return L.blame_of(L.decode(_image(names, 4, recs, len(recs)), names, widths, 4), row_len, record)

    assert blame(clean) is None
    # forward before gradient, and the FIRST site in forward order
    e = dict(clean)
    e[(0, 2)], e[(0, 1)], e[(1, 3)] = (10, 5, 3, 1.0, 1.0), (10, 2, 2 * 12 + 7, 1.0, 1.0), (10, 9, 0, 1.0, 1.0)
    assert blame(e) == {"half": "forward", "site": "b", "sample": 2, "position": 7, "n_bad": 2}
    # a clean forward: the first site in BACKWARD order whose gradient half is bad
    e = dict(clean)
    e[(1, 0)], e[(1, 2)] = (10, 1, 5, 1.0, 1.0), (10, 4, 9, 1.0, 1.0)
    assert blame(e) == {"half": "gradient", "site": "c", "sample": 2, "position": 1, "n_bad": 4}
    # an absent entry (have = 0) is never blamed, whatever its words hold; record= picks the record
    e = dict(clean)
    del e[(1, 3)]
    bad = dict(clean)
    bad[(0, 0)] = (10, 1, 21, 1.0, 1.0)
    assert blame(e, extra=[(0, 3, bad)]) is None
    assert blame(e, record=0, extra=[(0, 3, bad)]) == {"half": "forward", "site": "a", "sample": 1, "position": 1, "n_bad": 1}


# ------------------------------------------------------------------------------------------------------------ the site table
def test_site_table_of_a_1_1_and_a_2_2_model():
    from hri_emo_amd.train import ActivationLog, activation_site_names
    m1, m2 = _model(1), _model(2)
    l1 = ActivationLog.for_model(m1, capacity=2, device="cpu")
    assert l1.names == NAMES_1 == activation_site_names(1, 1)
    l2 = ActivationLog.for_model(m2, device="cpu")
    assert len(l2.names) == 23 and l2.capacity == 16 and l2.every == 1
    assert l2.names[:2] == ["input.audio", "input.text"] and l2.names[2:8] == NAMES_1[2:8]
    assert l2.names[8:14] == [n.replace("enc0", "enc1") for n in NAMES_1[2:8]]
    assert l2.names[14:] == ["gate.w", "gate.fused", "dec0.self", "dec0.cross", "dec0.ffn", "dec1.self", "dec1.cross", "dec1.ffn", "logits"]
    assert l2.widths == [64] * 22 + [4]
    # the sub-layers' dropout site ids are the keys
    enc1, dec1 = m2.cross_modal.layers[1], m2.emotion_decoder.layers[1]
    assert l2.names[l2.index[enc1._site[3]]] == "enc1.audio_ffn" and l2.names[l2.index[enc1._site[4]]] == "enc1.text_cross"
    assert l2.names[l2.index[dec1._site[1]]] == "dec1.cross" and l2.names[l2.index["logits"]] == "logits"
    assert l2.names[l2.index[("input", m2.cross_modal.layers[0]._site[1])]] == "input.text"
    # the MOSEI wrapper: the backbone's table
    from hri_emo_amd import MoseiFusionWithEmotionDecoder
    mm = MoseiFusionWithEmotionDecoder(d_audio=10, d_text=12, d_model=64, num_emotions=6, n_heads=2, num_layers_fusion=1,
                                       num_layers_decoder=1, beta_hidden=32)
    lm = ActivationLog.for_model(mm, device="cpu")
    assert lm.names == NAMES_1 and lm.widths[-1] == 6


def test_sites_patterns_and_refusals():
    from hri_emo_amd import _ops
    from hri_emo_amd.train import ActivationLog
    m = _model(2)
    pats = ["enc*.audio_ffn", "enc*.text_ffn", "gate.fused", "dec*.ffn", "logits"]
    log = ActivationLog.for_model(m, sites=pats, device="cpu")
    assert log.selected == ["enc0.audio_ffn", "enc0.text_ffn", "enc1.audio_ffn", "enc1.text_ffn", "gate.fused", "dec0.ffn", "dec1.ffn", "logits"]
    assert len(log.names) == 23                                    # the record keeps every site's words
    assert sorted(log.names[i] for i in set(log.index.values())) == sorted(log.selected)
    assert m.cross_modal.layers[0]._site[0] not in log.index and "gate.w" not in log.index      # not selected: no probe
    with pytest.raises(ValueError) as e:
        ActivationLog.for_model(m, sites=["enc0.audio_ffn", "enc7.nope"], device="cpu")
    assert "enc7.nope" in str(e.value) and "dec1.cross" in str(e.value)                          # the valid names are listed
    from hri_emo_amd import FusionClassifier
    with pytest.raises(NotImplementedError, match="FusionClassifier"):
        ActivationLog.for_model(FusionClassifier(d_model=64, num_classes=4, n_heads=2, num_layers=1), device="cpu")
    with pytest.raises(NotImplementedError, match="BetaGate"):
        ActivationLog.for_model(m.beta_gate, device="cpu")
    with pytest.raises(ValueError):
        ActivationLog.for_model(m, capacity=0, device="cpu")
    # fp32 precision: refused by name before anything is enqueued (CPU tensors would be refused later, by the first launch)
    was = _ops.precision()
    _ops.set_precision("fp32")
    try:
        with pytest.raises(NotImplementedError, match="fp32"):
            with log.watch():
                pass
        ctx = _ops.StepContext()
        ctx.act_log = log
        with _ops.use_context(ctx):
            with pytest.raises(NotImplementedError, match="fp32"):
                m(torch.randn(2, 6, 64), torch.randn(2, 4, 64))
    finally:
        _ops.set_precision(was)
    assert _ops.CTX.act_log is None
    with log.watch():
        assert _ops.CTX.act_log is log
        with log.paused():
            assert log.recording is False
        assert log.recording is True
    assert _ops.CTX.act_log is None and _ops.StepContext().act_log is None


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_entries_and_launcher_refusals():
    import ctypes
    from hri_emo_amd import _lib
    L = _lib.lib()
    assert L.hriemo_act_probe_rows() == R.ROWS
    from hri_emo_amd.train import ACT_PROBE_ROWS
    assert ACT_PROBE_ROWS == R.ROWS
    buf = (ctypes.c_int * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    ctr, win, cnt, ring, part, x = base, base + 16, base + 32, base + 256, base + 4096, base + 8192
    err = lambda: L.hriemo_last_error().decode()          # noqa: E731
    # (every call is refused in front of its launch: nothing here needs a GPU)
    assert L.hriemo_act_log_plan(2, 1, 1, 2, ctr, win, cnt, ring, None) != 0 and "record" in err()
    assert L.hriemo_act_log_plan(1, 0, 1, 2, ctr, win, cnt, ring, None) != 0 and "every" in err()
    assert L.hriemo_act_log_plan(1, 1, 0, 2, ctr, win, cnt, ring, None) != 0 and "capacity" in err()
    assert L.hriemo_act_log_plan(1, 1, 1, 2, ctr, ctr, cnt, ring, None) != 0 and "overlap" in err()
    assert L.hriemo_act_log_plan(1, 1, 1, 2, ctr + 4, win, cnt, ring, None) != 0 and "aligned" in err()
    probe = lambda **k: L.hriemo_act_probe(*[{**dict(x=x, dtype=0, n_rows=8, d=8, ld=8, cu=None, kpm=None, B=2, L=4, nv=None, win=win,      # noqa: E731
                                                     site=0, half=0, S=2, cap=4, part=part, cnt=cnt, st=None), **k}[n]
                                             for n in ("x", "dtype", "n_rows", "d", "ld", "cu", "kpm", "B", "L", "nv", "win", "site", "half", "S",
                                                       "cap", "part", "cnt", "st")])
    assert probe(dtype=2) != 0 and "dtype" in err()
    assert probe(ld=7) != 0 and "ld" in err()
    assert probe(n_rows=9) != 0 and "padded rows" in err()
    assert probe(site=2) != 0 and "site" in err()
    assert probe(half=2) != 0 and "half" in err()
    assert probe(n_rows=8 * R.ROWS, B=8 * R.ROWS, cap=7) != 0 and "chunks" in err()
    assert probe(cu=cnt, kpm=x) != 0 and "key_padding_mask" in err()
    assert probe(x=None) != 0 and "required" in err()
    assert probe(part=x) != 0 and "overlap" in err()
    assert L.hriemo_act_log_fold(part, cnt, win, 2, 2, 4, 1, ring, None) != 0 and "half" in err()
    assert L.hriemo_act_log_fold(part, cnt, win, 0, 2, 4, 0, ring, None) != 0 and "capacity" in err()
    assert L.hriemo_act_log_fold(ring, cnt, win, 0, 2, 4, 1, ring, None) != 0 and "overlap" in err()


# ------------------------------------------------------------------------------------------------------------ the reference
def test_reference_row_selection_and_statistics():
    """the reference's rules on hand-counted cases, and its constants against the package's"""
    from hri_emo_amd import _lib
    from hri_emo_amd.train import ACT_PROBE_ROWS
    assert R.ROWS == ACT_PROBE_ROWS == _lib.lib().hriemo_act_probe_rows()
    L = 4
    # packed: lengths (1, 3, 2) + a filler sequence + surplus rows; B = 3 real sequences
    cu = [0, 1, 4, 6, 8]
    rows = R.counted_rows(10, 3, L, cu=cu)
    assert rows.tolist() == [0, 4, 5, 6, 8, 9, -1, -1, -1, -1]
    assert R.counted_rows(10, 3, L, cu=cu, n_valid=2).tolist() == [0, 4, 5, 6, -1, -1, -1, -1, -1, -1]
    assert R.counted_rows(10, 3, L, cu=cu, n_valid=0).tolist()[:2] == [0, -1]                  # clamp(n_valid, 1, B)
    kpm = np.array([[0, 0, 1, 1], [0, 1, 0, 0]])                                                # the second mask is no prefix
    assert R.counted_rows(8, 2, L, kpm=kpm).tolist() == [0, 1, -1, -1, 4, -1, 6, 7]
    assert R.counted_rows(8, 2, L, n_valid=1).tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    x = torch.zeros(10, 8)
    x[1, 3], x[5, 7], x[2, 0], x[7, 0], x[9, 1] = float("nan"), float("inf"), -3.0, float("nan"), float("inf")
    x[4, 2] = 2.0
    ref = R.probe_ref64(x, 3, L, cu=cu)
    assert ref == {"n_rows": 6, "n_bad": 2, "first_bad_row": 4, "absmax": 3.0, "sumsq": 13.0}   # rows 7, 9: filler / surplus
    assert R.probe_ref64(torch.zeros(3, 8), 3, 1)["first_bad_row"] == -1
    # the tree the bound counts
    assert R.vec_of(torch.bfloat16, 776) == 8 and R.vec_of(torch.float32, 4) == 4 and R.vec_of(torch.float32, 6) == 1
    assert R.vec_of(torch.bfloat16, 8, 12) == 1
    assert R.roundings(65, 776, 8) == 8 * 13 + 9 + 1 + 9 and R.roundings(1, 8, 8) == 8 + 19
    assert R.sumsq_bound(1.0, 65, 776, 8) < 7.5e-6


def test_reference_stays_inside_its_own_bound_with_room():
    """float32 sequential summation of the test operands against the float64 reference: the scale the GPU tests draw (randn) keeps
    even a worse tree than the kernel's far inside the counted bound; the host decode turns the same sum into the rms it reports"""
    from hri_emo_amd.train import ActivationLog
    torch.manual_seed(0)
    for d in (8, 64, 776):
        x = torch.randn(2 * R.ROWS + 1, d).bfloat16()
        R.assert_no_underflow(x)
        ref = R.probe_ref64(x, 2 * R.ROWS + 1, 1)
        # pairwise fp32 (torch's sum) of exact squares: an independent fp32 route
        got = float((x.float() * x.float()).sum())
        assert abs(got - ref["sumsq"]) <= 0.5 * R.sumsq_bound(ref["sumsq"], x.shape[0], d, 8)
        img = _image(["s"], 1, [(0, 1, {(0, 0): (x.shape[0], 0, -1, ref["absmax"], got)})], 1)
        rms = ActivationLog.decode(img, ["s"], [d], 1)["forward"]["rms"][0, 0]
        assert rms == np.sqrt(float(np.float32(got)) / (x.shape[0] * d)) and abs(rms - 1.0) < 0.1      # randn rows: rms near 1
