"""CPU: the one host registry of the sync buffers handed to the launches that synchronise their work-groups in flight
(functional._SYNC: query-GRU chains, STN head, LSTM chain) -- what sync_check() and qgru_chain_check() read, and who holds the buffers."""
import copy
import gc

import pytest
import torch

from tatt_amd import functional as Fh
from tatt_amd import infer


@pytest.fixture
def registry(monkeypatch):
    """an empty registry, no sticky words, and buffer lookups that do not ask for a GPU"""
    monkeypatch.setattr(Fh, "_SYNC", [])
    monkeypatch.setattr(Fh, "_STICKY", {})
    monkeypatch.setattr(Fh, "sticky_word", lambda device: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return Fh._SYNC


REF = torch.zeros(1)


class _Holder:
    pass


def _one_of_each():
    holder = _Holder()
    return holder, Fh._qgru_chain_sync(REF).zero_(), Fh._stn_sync(holder, "f0", REF), infer._lstm_sync(REF)


def test_buffers_of_each_kind_are_registered_and_zeros_pass(registry):
    holder, q, s, l = _one_of_each()
    assert (q.numel(), s.numel(), l.numel()) == (1024, 256, 1024) and q.dtype == s.dtype == l.dtype == torch.int32
    assert [(r() is b, err) for (r, err, _), b in zip(registry, (q, s, l))] == [(True, 1023), (True, 255), (True, 1023)]
    Fh.sync_check()
    Fh.qgru_chain_check()


@pytest.mark.parametrize("kind,words", [(0, ("query-GRU",)), (1, ("STN-head",)), (2, ("LSTM", "tatt_lstm_fwd_chain"))])
def test_error_word_raises_with_the_family_s_words(registry, kind, words):
    holder, *bufs = _one_of_each()
    errs = (1023, 255, 1023)
    for b, err in zip(bufs, errs):                                  # every other word is somebody's flag: ignored
        b.fill_(7)
        b[err] = 0
    Fh.sync_check()
    bufs[kind][errs[kind]] = 1
    with pytest.raises(RuntimeError, match="gave up waiting") as e:
        Fh.sync_check()
    assert all(w in str(e.value) for w in words)
    assert sum(w in str(e.value) for w in ("query-GRU", "STN-head", "LSTM")) == 1


def test_qgru_chain_check_looks_at_query_gru_buffers_only(registry):
    holder, q, s, l = _one_of_each()
    s[255] = 1
    l[1023] = 1
    Fh.qgru_chain_check()
    with pytest.raises(RuntimeError, match="gave up waiting"):
        Fh.sync_check()
    q[1023] = 1
    with pytest.raises(RuntimeError, match="query-GRU"):
        Fh.qgru_chain_check()


def test_sticky_word_is_read_first(registry, monkeypatch):
    holder, q, s, l = _one_of_each()
    s[255] = 1
    monkeypatch.setattr(Fh, "_STICKY", {0: torch.tensor([1 | 4, 0, 0, 0], dtype=torch.int32)})
    with pytest.raises(RuntimeError, match=r"cuda:0 \(query-GRU chain \+ LSTM chain\)"):
        Fh.sync_check()


def test_stn_and_lstm_buffers_are_held_weakly_and_registered_once(registry):
    holder = _Holder()
    s = Fh._stn_sync(holder, "f0", REF)
    assert Fh._stn_sync(holder, "f0", REF) is s and Fh._stn_sync(holder, "f0", REF) is s
    assert Fh._stn_sync(holder, "b0", REF) is not s
    assert len(registry) == 2
    clone = copy.deepcopy(holder)                                   # brings its buffers unregistered: registered on lookup
    assert len(registry) == 2
    c = Fh._stn_sync(clone, "f0", REF)
    assert c is not s and len(registry) == 3 and Fh._stn_sync(clone, "f0", REF) is c and len(registry) == 3
    l = infer._lstm_sync(REF)
    assert len(registry) == 4
    s[255] = 1
    del s, holder                                                   # the module goes, and its buffers with it
    gc.collect()
    assert sum(r() is not None for r, _, _ in registry) == 2
    Fh.sync_check()                                                 # (a dead entry is skipped, its raised word is gone with it)
    del l
    gc.collect()
    l2 = infer._lstm_sync(REF)                                      # the next registration prunes the dead entries
    assert [id(r()) for r, _, _ in registry] == [id(c), id(l2)]


def test_query_gru_buffers_are_held_strongly_and_the_ninth_evicts_the_first(registry):
    holder = _Holder()
    s = Fh._stn_sync(holder, "f0", REF)
    ids = []
    for k in range(8):
        ids.append(id(Fh._qgru_chain_sync(REF).zero_()))            # nobody else keeps them
    gc.collect()
    assert [id(r()) for r, _, name in registry if "query-GRU" in name] == ids
    registry[1][0]()[1023] = 1                                      # the first query-GRU buffer gave up ...
    with pytest.raises(RuntimeError, match="query-GRU"):
        Fh.qgru_chain_check()
    ninth = Fh._qgru_chain_sync(REF).zero_()
    assert [id(r()) for r, _, name in registry if "query-GRU" in name] == ids[1:] + [id(ninth)]
    Fh.qgru_chain_check()                                           # ... and is gone with the ninth registration
    assert registry[0][0]() is s                                    # entries of the other kinds are not counted and not evicted
