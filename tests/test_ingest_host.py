"""CPU suite of the packed front door: `data.collate_seq_packed`, the plans `forward_packed` builds from lengths alone, and its
argument checks -- none of which touches a device."""
import pytest
import torch

from conftest import load_golden


def _collate_batch(g):
    return [(g[f"xa{i}"], g[f"ka{i}"], g[f"xt{i}"], g[f"kt{i}"], g[f"y{i}"]) for i in range(4)]


def test_collate_seq_packed_is_collate_seq_batch_gathered_at_the_valid_rows():
    """the reference's recorded collate (tests/golden/collate.npz): the packed collate hands over exactly the rows the padded batch
    holds at its valid positions, in batch order, and the lengths the masks count; labels of both loss types unchanged"""
    from hri_emo_amd import data
    g = load_golden("collate")
    batch = _collate_batch(g)
    rows_a, len_a, rows_t, len_t, labels = data.collate_seq_packed(batch, "multi_label")
    h_a, m_a, h_t, m_t, ref_labels = data.collate_seq_batch(batch, "multi_label")
    assert torch.equal(h_a, g["h_a"]) and torch.equal(m_a, g["mask_a"])          # (the padded collate is the fixture's)
    assert torch.equal(rows_a, g["h_a"][~g["mask_a"]]) and torch.equal(rows_t, g["h_t"][~g["mask_t"]])
    assert torch.equal(len_a, (~g["mask_a"]).sum(1)) and torch.equal(len_t, (~g["mask_t"]).sum(1))
    assert len_a.dtype == torch.int64 and not len_a.is_cuda
    assert rows_a.shape == (int(len_a.sum()), 16) and rows_t.shape == (int(len_t.sum()), 16)
    assert torch.equal(labels, ref_labels) and torch.equal(labels, g["labels"])
    single = data.collate_seq_packed([(b[0], b[1], b[2], b[3], i % 4) for i, b in enumerate(batch)], "single_label")[4]
    assert torch.equal(single, g["single"])


@pytest.mark.parametrize("la,lt,La,Lt", [([70, 33, 32, 1, 17], [40, 1, 32, 31, 16], 70, 40),
                                         ([48, 10, 33], [20, 17, 5], 48, 20),
                                         ([3, 2], [3, 1], 9, 4),                    # pad_to beyond the batch maxima
                                         ([1], [1], 1, 1)])
def test_plans_from_lengths_equal_the_plans_of_the_masks(la, lt, La, Lt):
    """_ops.plans_from_lengths against _ops.seq_plans of the corresponding prefix masks: cu, L, Lmax, N of the three plans, the
    fused lengths min(la, lt), and the masks themselves"""
    from hri_emo_amd import _ops
    B = len(la)
    m_a = torch.arange(La)[None] >= torch.tensor(la)[:, None]
    m_t = torch.arange(Lt)[None] >= torch.tensor(lt)[:, None]
    ref = _ops.seq_plans(m_a, m_t, B, La, Lt)
    got, masks = _ops.plans_from_lengths(la, lt, La, Lt, torch.device("cpu"))
    assert torch.equal(masks[0], m_a) and torch.equal(masks[1], m_t) and masks[0].dtype == torch.bool
    for s, r in zip(got, ref):
        assert torch.equal(s.cu, r.cu) and s.cu.dtype == torch.int32
        assert (s.B, s.Breal, s.L, s.Lmax, s.N, s.surplus, s.kpm) == (r.B, r.Breal, r.L, r.Lmax, r.N, r.surplus, r.kpm)
    lf = (got[2].cu[1:] - got[2].cu[:-1]).tolist()
    assert lf == [min(x, y) for x, y in zip(la, lt)]
    assert got[0].idx.shape == ref[0].idx.shape and got[0].idx.dtype == torch.int64 and got[2].idx is None and ref[2].idx is None
    # (idx of the two modality plans is written by the ingest launch; the padded rows it must hold are the mask plan's)
    assert ref[0].idx.tolist() == [b * La + l for b in range(B) for l in range(la[b])]
    again, _ = _ops.plans_from_lengths(la, lt, La, Lt, torch.device("cpu"))
    assert again[0] is got[0]                                                       # cached per (lengths, pad_to, device)


def test_forward_packed_argument_checks_raise_on_the_host():
    """every refusal of forward_packed comes before anything touches a device: CPU models, CPU rows"""
    import hri_emo_amd as H
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, num_layers_fusion=1, num_layers_decoder=1)
    ra, rt = torch.zeros(5, 128), torch.zeros(4, 128)
    with pytest.raises(ValueError, match="outside"):
        m.forward_packed(ra, rt, [5, 0], [3, 1])                                    # a zero length
    with pytest.raises(ValueError, match="outside"):
        m.forward_packed(ra, rt, [3, 2], [3, 1], pad_to=(2, 2))                     # longer than pad_to
    with pytest.raises(ValueError, match="outside"):
        m.forward_packed(ra, rt, torch.tensor([6, -1]), torch.tensor([3, 1]))
    with pytest.raises(RuntimeError, match="L_t"):
        m.forward_packed(rt, ra, [2, 2], [3, 2])                                    # L_t > L_a, the reference gate's refusal
    with pytest.raises(RuntimeError, match="L_t"):
        m.forward_packed(ra, rt, [3, 2], [3, 1], pad_to=(3, 4))
    with pytest.raises(ValueError, match="lengths"):
        m.forward_packed(ra, rt, [3, 2], [3, 1, 1])
    with pytest.raises(ValueError, match="sum"):
        m.forward_packed(ra, rt, [3, 1], [3, 1])                                    # rows do not add up
    with pytest.raises(ValueError, match="sum"):
        m.forward_packed(ra.view(1, 5, 128), rt, [3, 2], [3, 1])                    # not [N, d]
    with pytest.raises(ValueError, match="dtype"):
        m.forward_packed(ra.double(), rt.double(), [3, 2], [3, 1])
    with pytest.raises(ValueError, match="differ"):
        m.forward_packed(ra, rt.half(), [3, 2], [3, 1])
    H.set_varlen_maps(False)
    with pytest.raises(ValueError, match="set_varlen_maps"):
        m.forward_packed(ra, rt, [3, 2], [3, 1], return_attention=True)
    with pytest.raises(RuntimeError, match="MI355X"):                               # valid arguments: only now the device matters
        m.forward_packed(ra, rt, [3, 2], [3, 1])
    w = H.MoseiFusionWithEmotionDecoder(d_audio=74, d_text=300, d_model=128, n_heads=8, num_layers_fusion=1, num_layers_decoder=1)
    with pytest.raises(ValueError, match="outside"):
        w.forward_packed(torch.zeros(5, 74), torch.zeros(4, 300), [5, 0], [3, 1])
    with pytest.raises(RuntimeError, match="L_t"):
        w.forward_packed(torch.zeros(4, 74), torch.zeros(5, 300), [2, 2], [3, 2])


def test_ingest_switch_ships_off_and_round_trips():
    import hri_emo_amd as H
    from hri_emo_amd import _ops
    assert H.ingest() is False and _ops.INGEST_ROWS is False
    H.set_ingest(True)
    try:
        assert H.ingest() is True and _ops.ingestible(torch.zeros(1), torch.zeros(1, dtype=torch.float16))
        assert not _ops.ingestible(torch.zeros(1, dtype=torch.float64))
    finally:
        H.set_ingest(False)
    assert not _ops.ingestible(torch.zeros(1))
