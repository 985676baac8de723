"""CPU suite of train.AttentionLog: the window rule of hriemo_attn_log_plan against a ten-line Python model, as_reference against
the committed CPU oracle's own per-batch maps (pure data movement: np.array_equal, no tolerance), the refusals and nbytes.  All of
it runs on the CPU twin of the log; tests/test_gpu_attention_log_kernels.py runs the same sequences through the kernels."""
import numpy as np
import pytest
import torch

from oracle import hri_emo_oracle as O          # the checker (tests only)

SITES = ("audio_self", "text_self", "audio_queries_text", "text_queries_audio")
#            capacity, [(B, n_valid | None)]
SEQUENCES = {
    "5, 5, 5, 3 into 12": (12, [(5, None), (5, None), (5, None), (3, None)]),
    "capacity below B": (3, [(5, None), (5, None)]),
    "short batches": (12, [(5, 3), (5, 1), (5, None), (5, 4), (5, 2)]),
    "n_valid out of range is clamped": (7, [(5, 0), (5, 9), (5, -3)]),
}


def model_plan(state, capacity, B, n_valid, lens):
    """the rule, in ten lines: state = dict(cursor, n_offered, n_batches, lengths [2, capacity]) -> the window (slot0, n_take)"""
    nv = B if n_valid is None else min(max(n_valid, 1), B)
    cur = state["cursor"]
    take = min(capacity - cur, nv) if 0 <= cur <= capacity else 0
    for b in range(take):
        state["lengths"][:, cur + b] = lens[:, b]
    state["cursor"] = cur + take
    state["n_offered"] += nv
    state["n_batches"] += 1
    return cur, take


def fresh(capacity):
    return {"cursor": 0, "n_offered": 0, "n_batches": 0, "lengths": np.zeros((2, capacity), dtype=np.int32)}


def lens_of(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(1, 9, (B,), generator=g), torch.randint(1, 5, (B,), generator=g)]).to(torch.int32)


def _log(capacity, **kw):
    from hri_emo_amd.train import AttentionLog
    return AttentionLog(capacity, (8, 4), 1, 1, 3, device="cpu", **kw)


def _agree(log, state, win, what):
    assert log.window.tolist() == [win[0], win[1], 0, 0], (what, log.window.tolist(), win)
    assert log.counters.tolist() == [state["cursor"], state["n_offered"], state["n_batches"], 0], (what, log.counters.tolist(), state)
    assert np.array_equal(log.lengths.numpy(), state["lengths"]), what


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_window_rule_against_the_python_model(name):
    capacity, seq = SEQUENCES[name]
    log, state = _log(capacity), fresh(capacity)
    takes = []
    for i, (B, nv) in enumerate(seq):
        lens = lens_of(B, 100 + i)
        log.plan(lens, nv)
        win = model_plan(state, capacity, B, nv, lens.numpy())
        takes.append(win[1])
        _agree(log, state, win, (name, i))
    if name == "5, 5, 5, 3 into 12":
        assert takes == [5, 5, 2, 0] and log.counters.tolist() == [12, 18, 4, 0]
    if name == "capacity below B":
        assert takes == [3, 0]
    # reset(): the counters and the window start over, the next batch lands in slot 0
    log.reset()
    state.update(cursor=0, n_offered=0, n_batches=0)
    assert log.counters.tolist() == [0, 0, 0, 0]
    lens = lens_of(2, 7)
    log.plan(lens)
    _agree(log, state, model_plan(state, capacity, 2, None, lens.numpy()), (name, "after reset"))


@pytest.mark.parametrize("cursor", [-1, 13], ids=["-1", "capacity + 1"])
def test_a_corrupt_cursor_takes_nothing(cursor):
    log, state = _log(12), fresh(12)
    log.plan(lens_of(5, 1))
    model_plan(state, 12, 5, None, lens_of(5, 1).numpy())
    log.counters[0] = cursor
    state["cursor"] = cursor
    maps = log.decoder_maps[0].clone()
    lens = lens_of(5, 2)
    log.plan(lens, 4)
    win = model_plan(state, 12, 5, 4, lens.numpy())
    assert win == (cursor, 0)
    _agree(log, state, win, "corrupt cursor")          # only n_offered, n_batches and the window moved
    log._append_one(torch.ones(5, 3, 4), log.decoder_maps[0])
    assert torch.equal(log.decoder_maps[0], maps)
    assert log.arrays()["n_logged"] == (0 if cursor < 0 else 12)


def test_the_closed_window_touches_nothing_else():
    log = _log(6)
    log.plan(lens_of(4, 3))
    before = (log.counters.clone(), log.lengths.clone())
    log.plan(lens_of(4, 4), record=False)
    assert log.window.tolist() == [0, 0, 0, 0]
    assert torch.equal(log.counters, before[0]) and torch.equal(log.lengths, before[1])
    maps = log.decoder_maps[0].clone()
    log._append_one(torch.ones(4, 3, 4), log.decoder_maps[0])
    assert torch.equal(log.decoder_maps[0], maps)


# ----------------------------------------------------------------------------- as_reference against the oracle
D, NE, LA, LT = 32, 3, 11, 7
BATCHES = [([11, 3, 6], [5, 1, 4]), ([2, 9], [2, 7])]          # (audio lengths, text lengths): two ragged batches, own padding each


def _oracle_batches():
    torch.manual_seed(5)
    ref = O.closed_form_init_(O.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=4, dropout=0.0)).eval()
    out = []
    g = torch.Generator().manual_seed(9)
    for la, lt in BATCHES:
        B, ma, mt = len(la), max(la), max(lt)          # pad to the batch's own maxima, as the reference's collate does
        h_a, h_t = torch.randn(B, ma, D, generator=g), torch.randn(B, mt, D, generator=g)
        mask_a = torch.arange(ma)[None] >= torch.tensor(la)[:, None]
        mask_t = torch.arange(mt)[None] >= torch.tensor(lt)[:, None]
        with torch.no_grad():
            pack = ref(h_a, h_t, mask_a, mask_t, return_attention=True)[3]
        out.append((la, lt, pack))
    return out


def _pad(x, Lq, Lk):
    out = torch.zeros(x.shape[0], Lq, Lk)
    out[:, :x.shape[1], :x.shape[2]] = x
    return out


def test_as_reference_is_the_oracles_collected_attns():
    from hri_emo_amd.train import AttentionLog
    batches = _oracle_batches()
    log = AttentionLog(8, (LA, LT), 2, 2, NE, device="cpu")
    dims = dict(zip(SITES, ((LA, LA), (LT, LT), (LA, LT), (LT, LA))))
    for la, lt, pack in batches:
        # the packed export's form of these maps: padded to pad_to, PAD query rows zero (the oracle computes those rows)
        enc = []
        for layer in pack["encoder"]:
            d = {}
            for k in SITES:
                m = layer[k].float().clone()
                ql = la if k in ("audio_self", "audio_queries_text") else lt
                for b, n in enumerate(ql):
                    m[b, n:] = 0
                d[k] = _pad(m, *dims[k])
            enc.append(d)
        dec = [_pad(t.float(), NE, LT) for t in pack["decoder"]]
        log.append({"encoder": enc, "decoder": dec}, torch.tensor([la, lt], dtype=torch.int32))
    got = log.as_reference(3)          # the first batch had 3 samples, the second 2: the reference's batches again
    assert len(got["encoder"]) == len(got["decoder"]) == 2
    for (la, lt, pack), enc, dec in zip(batches, got["encoder"], got["decoder"]):
        assert len(enc) == 2 and len(dec) == 2
        for layer_ref, layer in zip(pack["encoder"], enc):
            assert tuple(layer) == SITES
            for k in SITES:
                ref = layer_ref[k].float().numpy()
                assert layer[k].shape == ref.shape and layer[k].dtype == np.float32, (k, layer[k].shape, ref.shape)
                ql = la if k in ("audio_self", "audio_queries_text") else lt
                for b, n in enumerate(ql):
                    assert np.array_equal(layer[k][b, :n], ref[b, :n]), (k, b)
                    assert not layer[k][b, n:].any(), (k, b, "PAD query rows are zeros")
        for ref, mine in zip(pack["decoder"], dec):
            assert mine.shape == tuple(ref.shape) and np.array_equal(mine, ref.float().numpy())
    arr = log.arrays()
    assert arr["n_logged"] == 5 and arr["n_offered"] == 5
    assert arr["lengths"].tolist() == [[11, 3, 6, 2, 9], [5, 1, 4, 2, 7]]
    assert arr["encoder"][0]["audio_queries_text"].shape == (5, LA, LT) and arr["decoder"][1].shape == (5, NE, LT)


def test_halves_can_be_switched_off():
    dec_only = _log(4, encoder=False)
    assert dec_only.encoder_maps == [] and len(dec_only.decoder_maps) == 1
    dec_only.append({"encoder": None, "decoder": [torch.ones(2, 3, 4)]}, torch.tensor([[8, 2], [4, 1]], dtype=torch.int32))
    ref = dec_only.as_reference(2)
    assert ref["encoder"] == [] and ref["decoder"][0][0].shape == (2, 3, 4)
    enc_only = _log(4, decoder=False)
    assert enc_only.decoder_maps == [] and tuple(enc_only.encoder_maps[0]) == SITES
    assert enc_only.sites(2)[1] is None and dec_only.sites(2)[0] is None


# ----------------------------------------------------------------------------- refusals, nbytes
def test_constructor_refusals():
    from hri_emo_amd.train import AttentionLog
    good = dict(capacity=4, pad_to=(8, 4), num_layers_fusion=1, num_layers_decoder=1, num_emotions=3, device="cpu")
    AttentionLog(**good)
    for what, change in {"capacity 0": dict(capacity=0), "pad_to of one": dict(pad_to=(8,)), "pad_to no pair": dict(pad_to=8),
                         "L_t > L_a": dict(pad_to=(4, 8)), "L_t 0": dict(pad_to=(4, 0)), "no layers": dict(num_layers_fusion=0),
                         "no decoder layers": dict(num_layers_decoder=0), "no emotions": dict(num_emotions=0),
                         "neither half": dict(encoder=False, decoder=False)}.items():
        with pytest.raises(ValueError):
            AttentionLog(**dict(good, **change))
        assert what
    log = AttentionLog(**good)
    with pytest.raises(ValueError):
        log.plan(torch.zeros(2, 3))                                  # not int32
    with pytest.raises(ValueError):
        log.plan(None)                                               # no B
    with pytest.raises(ValueError):
        log.append({"encoder": [], "decoder": [torch.zeros(2, 3, 4)]}, torch.ones(2, 2, dtype=torch.int32))      # layer count
    with pytest.raises(ValueError):
        log.as_reference(0)
    assert log.counters.tolist() == [0, 0, 0, 0]


def test_for_model_reads_the_model_and_unwraps_the_mosei_wrapper():
    import hri_emo_amd as H
    from hri_emo_amd.train import AttentionLog
    m = H.FusionWithEmotionDecoder(d_model=32, num_emotions=5, n_heads=4, num_layers_fusion=3, num_layers_decoder=1)
    log = AttentionLog.for_model(m, 6, (9, 4))
    assert (log.num_layers_fusion, log.num_layers_decoder, log.num_emotions, log.device.type) == (3, 1, 5, "cpu")
    assert log.mismatch(m, (9, 4)) is None
    assert "pad_to" in log.mismatch(m, (9, 5))
    w = H.MoseiFusionWithEmotionDecoder(7, 9, d_model=32, num_emotions=6, n_heads=4, num_layers_fusion=1, num_layers_decoder=2)
    lw = AttentionLog.for_model(w, 6, (9, 4), encoder=False)
    assert (lw.num_layers_fusion, lw.num_layers_decoder, lw.num_emotions, lw.encoder) == (1, 2, 6, False)
    # (a half the log does not keep is not compared: lw has no encoder maps; the first mismatch found is named)
    assert lw.mismatch(w) is None and "num_layers_decoder" in lw.mismatch(m) and "num_layers_fusion" in log.mismatch(w)
    m6 = H.FusionWithEmotionDecoder(d_model=32, num_emotions=4, n_heads=4, num_layers_fusion=3, num_layers_decoder=2)
    assert "num_emotions" in lw.mismatch(m6)
    with pytest.raises(TypeError):
        AttentionLog.for_model(torch.nn.Linear(2, 2), 6, (9, 4))


@pytest.mark.parametrize("enc,dec", [(True, True), (False, True), (True, False)], ids=["both", "decoder only", "encoder only"])
def test_nbytes(enc, dec):
    from hri_emo_amd.train import AttentionLog
    cap, La, Lt, n_enc, n_dec, ne = 12, 70, 40, 2, 3, 4
    log = AttentionLog(cap, (La, Lt), n_enc, n_dec, ne, encoder=enc, decoder=dec, device="cpu")
    maps = 4 * cap * ((n_enc * (La * La + Lt * Lt + 2 * La * Lt) if enc else 0) + (n_dec * ne * Lt if dec else 0))
    small = 4 * (4 + 4 + 2 * cap)          # counters, window, lengths
    assert log.nbytes == maps + small
