"""CPU suite of the bucket-graph cache every captured ragged step shares (dp._PackedState.graph): LRU order and eviction at the cap,
the GRAPHS_ALIVE accounting through _GraphRecord.release, torch's CPU generator around a capture, a capture that fails, the one
memory pool.  The device is replaced by stubs; the capture callable does what _record_graph does to the counter."""
import logging
import types

import pytest
import torch


@pytest.fixture
def cache(monkeypatch):
    from hri_emo_amd import _ops, dp
    calls = types.SimpleNamespace(sync=0, pool=0, seqs=[])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: setattr(calls, "sync", calls.sync + 1))
    monkeypatch.setattr(torch.cuda, "graph_pool_handle", lambda: setattr(calls, "pool", calls.pool + 1) or ("pool", calls.pool))
    monkeypatch.setattr(_ops, "seq_bucket", lambda cu, B, L, rows: ("seq", B, L, rows))
    monkeypatch.setattr(_ops, "seq_bucket_fused", lambda cu, B, L, rows: ("fused", B, L, rows))
    monkeypatch.setattr(_ops, "GRAPHS_ALIVE", 5)            # graphs of somebody else: the counter never reaches zero here
    pb = dp._PackedState(2, 4, 3, "cpu")

    def capture(seqs):
        calls.seqs.append(seqs)
        torch.rand(3)                                       # the warm-up passes of a trainer's capture draw dropout seeds
        _ops.GRAPHS_ALIVE += 1
        return dp._GraphRecord(types.SimpleNamespace(), torch.zeros(()), [], seqs)

    def get(key, fn=capture):
        rec = pb.graph(key, 2, fn, "eval step")
        assert _ops.GRAPHS_ALIVE == 5 + len(pb.graphs)
        return rec

    return pb, get, calls


K1, K2, K3 = (8, 8), (16, 8), (16, 16)


def test_lru_order_eviction_and_accounting(cache, caplog):
    pb, get, calls = cache
    caplog.set_level(logging.INFO, logger="hri_emo_amd.dp")
    r1, r2 = get(K1), get(K2)
    assert calls.seqs == [(("seq", 2, 4, k[0]), ("seq", 2, 3, k[1]), ("fused", 2, 3, k[1])) for k in (K1, K2)]
    assert r1.seqs == calls.seqs[0] and pb.pool == ("pool", 1)
    r3 = get(K3)                                            # the third key at cap 2: the first-captured graph goes
    assert list(pb.graphs) == [K2, K3] and r1.graph is None and r2.graph is not None and calls.sync == 1
    assert get(K2) is r2 and list(pb.graphs) == [K3, K2], "a hit returns the same record and moves it to the end"
    assert len(calls.seqs) == 3 and calls.sync == 1, "a hit captures and releases nothing"
    r1b = get(K1)                                           # least recently USED goes first, not first captured
    assert list(pb.graphs) == [K2, K1] and r3.graph is None and r2.graph is not None and r1b is not r1 and calls.sync == 2
    assert calls.pool == 1 and pb.pool == ("pool", 1), "one pool for all bucket graphs"
    said = [r.getMessage() for r in caplog.records]
    assert said.count("eval step: released the graph of bucket (8, 8) (cap 2)") == 1
    assert said.count("eval step: captured the graph of bucket (audio rows, text rows) = (16, 16) (2 alive)") == 1


def test_cpu_generator_around_a_capture(cache):
    pb, get, _ = cache
    torch.manual_seed(11)
    start = torch.get_rng_state()
    get(K1)
    after_first = torch.get_rng_state()
    torch.set_rng_state(start)
    torch.rand(3)
    assert torch.equal(after_first, torch.get_rng_state()) and not torch.equal(after_first, start), "the first capture keeps its draws"
    get(K2)
    assert torch.equal(torch.get_rng_state(), after_first), "a bucket met later hands the generator back"
    get(K3)                                                 # with an eviction in front of the capture
    assert torch.equal(torch.get_rng_state(), after_first)
    get(K3)
    assert torch.equal(torch.get_rng_state(), after_first)


def test_a_failed_capture_leaves_no_entry(cache):
    pb, get, calls = cache
    get(K1)
    before = torch.get_rng_state()

    def boom(seqs):
        torch.rand(5)
        raise RuntimeError("capture failed")

    with pytest.raises(RuntimeError, match="capture failed"):
        get(K2, boom)
    from hri_emo_amd import _ops
    assert list(pb.graphs) == [K1] and _ops.GRAPHS_ALIVE == 6 and torch.equal(torch.get_rng_state(), before)
    r2 = get(K2)
    assert list(pb.graphs) == [K1, K2] and r2.graph is not None and calls.pool == 1
