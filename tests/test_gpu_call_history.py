"""No search's answer depends on the calls before it (docs/exactness.md, "Calls do not see each other").

The chain of a search keeps its bookkeeping in per-workspace and per-shard device memory that no memset clears in front of a call:
the kernels clean up behind themselves, on every path, early returns included.  The other GPU tests reach each rare path on a
fresh index or repeat one path; here ONE index per test takes the calls of tests/_call_circuit.py's palettes in an order in which
every ordered pair of call kinds occurs exactly once (`circuit(K)`: K*K + 1 calls), and after EVERY call the rows, the score bits,
the counts, the padded tail and the path the call reports must be what the same call gives as the first search of a fresh index.

* "fresh": every kind as the first search of its own index — the oracle's answer and the path the kind's name claims (a palette
  whose kinds do not reach their paths fails here);
* "host circuit": the calls through search / search_pred / count_exact;
* "short-chain circuit" (L, T): the cut described below;
* "device circuit" (L, T): through search_device on one stream into caller buffers poisoned before every call (ids 0xABAB...,
  scores 7.0, counts 9): a stale slot or an unwritten count shows.  search_pred and count_exact have no device form: a predicate
  kind runs as search_device with the bitmap its predicate selects, count_exact as the host call it is (it shares the shard);
* "two streams" (L): the calls alternate between two streams, hence two workspaces, the device idle between calls: an answer must
  not depend on which workspace served the previous call.

What was cut, and why.  On a shard of >= 2^18 rows a host call first enqueues the SHORT chain (qprep, sweep, select, rescore, final:
nmn_api.hip, host_batch_body).  When that comes back flagged — a first selection overflowed — the call is run again with the whole
chain, and the next 256 host calls enqueue the whole chain at once (short_off_until).  That rule is adaptive state, it fires in the
full host circuits of L and T at their first flagged kind (L: `crowd`, call 18; T: call 0), and from there on those circuits
enqueue what search_device enqueues: the reported path and the answer do not tell the two chains apart.  So the short chain — what
a fresh index and an undisturbed host caller run, with its own bookkeeping: select_kernel told that crowd kernels follow when
none does, the resets of fb_sync and crowd_ctr in that mode — gets a circuit of its own: the kinds whose call is never flagged
(`Palette.quiet_kinds()`: 14 of L's 18, 4 of T's 9), on an index of their own, where short_off_until never moves and every pair is
a pair of short-chain calls (kinds with k > 4096 and count_exact have one chain only).  A flagged call is BY DESIGN followed only by
whole-chain calls; the transitions out of a flagged kind therefore exist in that form alone, and the full circuits hold them.
S is below 2^18 rows: its host calls have one chain.

No other adaptive rule fires inside a circuit.  The mirrors' on/off switches look at their counters at every 256th search that
could read the mirror (nmn_api.hip: q8_calls / half_calls) and act only when more than half of those were retried: in L at most
seven of the 18 kinds count towards one switch, 126 of the 325 calls (two more for the calls the host API runs again); T's every
query overflows, but its circuit is 82 calls; S is below 2^18 rows, where nothing is counted.  Every test builds its own index,
so no count carries over.  `test_the_retry_kind_is_counted...` lets the bf16 switch fire on purpose, on its own index: it is how
the library itself tells that `retry_f32` reaches the f32 retry's selection and `near_bf16` does not.

No assertion here was tried against a broken kernel: a lost reset can walk a list past its end.  The argument that the test bites
is the pair coverage (tests/test_call_circuit_cpu.py) and the fingerprints.
"""
import contextlib

import numpy as np
import pytest

from tests import _call_circuit as cc

pytestmark = pytest.mark.gpu
POISON_ROW = 0xABABABABABABABAB - (1 << 64)      # the int64 with that bit pattern


@contextlib.contextmanager
def _shard(pal):
    """A fresh index holding the palette's rows (+ the integer column of its predicate kinds) -> (idx, columns, column id)."""
    from neumann_amd import GpuFlatIndex
    from neumann_amd import columns as g
    with contextlib.ExitStack() as stack:
        idx = stack.enter_context(GpuFlatIndex(pal.d, pal.n, **pal.index_kwargs))
        pal.populate(idx)
        cols, c = None, None
        if pal.tag is not None:
            cols = stack.enter_context(g.GpuColumns(pal.n))
            c = cols.add_column()
            cols.write(c, 0, np.full(pal.n, g.CELL_INT, np.uint8), pal.tag.astype(np.uint64))
            cols.write_valid(0, np.full((pal.n + 63) // 64, 0xFFFFFFFFFFFFFFFF, np.uint64))
        yield idx, cols, c


def _host_call(shard, kd):
    """One call of kind `kd` through the host API -> (answer, nmn_search_stats or None)."""
    idx, cols, c = shard
    idx.set_mirror(kd.mirror)
    if kd.op == "count":
        return idx.count_exact(kd.Q[0], kd.score, kd.metric), None
    if kd.op == "pred":
        rows, scores, counts, selected, st = idx.search_pred(cols, cc.pred_program(kd, c), [], kd.Q, kd.k, kd.metric, with_stats=True)
        assert selected == int(kd.keep.sum()), (kd.name, selected)
    else:
        rows, scores, counts, st = idx.search(kd.Q, kd.k, kd.metric, mask=kd.mask, with_stats=True)
    return (rows, scores, counts), st


class _DeviceCalls:
    """search_device of every kind into its own caller buffers, poisoned before every call."""

    def __init__(self, pal, shard):
        import torch
        self.torch, self.shard, self.bufs = torch, shard, {}
        for kd in pal.kinds:
            if kd.op == "count":
                continue
            q = torch.from_numpy(kd.Q).cuda()
            m = None if kd.mask is None else torch.from_numpy(kd.mask.view(np.int64)).cuda()
            out = (torch.empty((kd.nq, kd.k), dtype=torch.int64, device="cuda"),
                   torch.empty((kd.nq, kd.k), dtype=torch.float32, device="cuda"),
                   torch.empty((kd.nq,), dtype=torch.int32, device="cuda"))
            self.bufs[kd.name] = (q, m, out)
        torch.cuda.synchronize()

    def __call__(self, kd, stream):
        torch, (idx, _, _) = self.torch, self.shard
        if kd.op == "count":
            return _host_call(self.shard, kd)
        idx.set_mirror(kd.mirror)
        q, m, out = self.bufs[kd.name]
        with torch.cuda.stream(stream):
            out[0].fill_(POISON_ROW)
            out[1].fill_(7.0)
            out[2].fill_(9)
            idx.search_device(q, kd.k, kd.metric, mask_t=m, out=out, stream=stream)
        stream.synchronize()
        st = idx.last_stats(stream)
        return (out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)), st


def _path(pal, kd, st):
    return None if st is None else cc.fingerprint(st, pal.d, kd.crowd_min, kd.fits)


def _walk(pal, kinds, call, what):
    """The circuit over `kinds` through `call(kind, step) -> (answer, stats)`; every failure names the pair: the previous kind,
    then this kind."""
    order = cc.circuit(len(kinds))
    assert len(order) == len(kinds) ** 2 + 1
    failures, prev = [], "(fresh index)"
    for step, ki in enumerate(order):
        kd = kinds[ki]
        got, st = call(kd, step)
        pair = f"{prev} -> {kd.name} (call {step})"
        bad = cc.mismatch(kd, got)
        if bad is not None:
            failures.append(f"{pair}: answer: {bad}")
        if _path(pal, kd, st) != kd.fp:
            failures.append(f"{pair}: path {_path(pal, kd, st)}, as a first search {kd.fp}")
        prev = kd.name
    print(f"{what} {pal.name}: K = {len(kinds)}, {len(order)} calls")
    assert not failures, f"{what} {pal.name}: {len(failures)} failures, the first: " + " | ".join(failures[:12])


@pytest.mark.parametrize("name", ["L", "T", "S"])
def test_fresh_every_kind_as_a_first_search_takes_its_path_and_matches_the_oracle(name):
    pal = cc.palette(name)
    failures = []
    for kd in pal.kinds:
        with _shard(pal) as shard:
            got, st = _host_call(shard, kd)
        fp = _path(pal, kd, st)
        rescored = None if st is None else int(st.candidates_rescored)
        print(f"fresh {pal.name}.{kd.name}: {fp}, {rescored} candidates re-scored")
        bad = cc.mismatch(kd, got)
        if bad is not None:
            failures.append(f"{kd.name}: answer: {bad}")
        if fp != kd.fp:
            failures.append(f"{kd.name}: path {fp}, its name claims {kd.fp}")
        # a kind marked quiet must show no sign of an overflowed first selection (necessary, not sufficient: an f32 retry leaves
        # none — only `retry_f32` is built to take one, and the test below observes it)
        if st is not None and not kd.flags and pal.n >= 1 << 18 and (st.fallback_queries or rescored > 4096):
            failures.append(f"{kd.name}: marked as never flagged, but {st.fallback_queries} fallback queries, {rescored} re-scored")
    assert not failures, " | ".join(failures)


def test_the_retry_kind_is_counted_as_retried_and_the_near_kind_is_not():
    """What the fingerprint cannot show, read off the library's own counters.  select_kernel counts a query in half_stats[1] when
    the f32 retry's selection takes it (nmn_select.hip:201-206: not when the first selection stood, not when the crowd list took
    it); at the 256th search on the bf16 mirror the shard leaves the mirror if more than half were counted (nmn_api.hip,
    half_off_until) and sweeps the f32 rows.  So 300 calls of `retry_f32` end on 4 bytes per element, 300 calls of `near_bf16`
    stay on 2 — with the oracle's answer throughout.  (The first call of each is flagged and counts once as an overflow of the short
    chain; 1 of 256 moves nothing.)"""
    pal = cc.palette("L")
    for name, switches in (("retry_f32", True), ("near_bf16", False)):
        kd = pal.kind(name)
        with _shard(pal) as shard:
            seen = []
            for i in range(300):
                got, st = _host_call(shard, kd)
                seen.append(cc.fingerprint(st, pal.d)[1])
                assert st.fallback_queries == 0 and cc.mismatch(kd, got) is None, (name, i, cc.mismatch(kd, got))
        print(f"{name}: bytes per element {seen[0]} -> {seen[-1]}, first call on {seen[-1]}: {seen.index(seen[-1])}")
        assert seen[0] == 2 and set(seen) == ({2, 4} if switches else {2}) and seen[-1] == (4 if switches else 2), (name, sorted(set(seen)))
        assert not switches or seen == sorted(seen), name      # switched once, did not come back


@pytest.mark.parametrize("name", ["L", "T", "S"])
def test_host_circuit_every_call_answers_as_on_a_fresh_index(name):
    pal = cc.palette(name)
    with _shard(pal) as shard:
        _walk(pal, pal.kinds, lambda kd, step: _host_call(shard, kd), "host circuit")


@pytest.mark.parametrize("name", ["L", "T"])
def test_short_chain_circuit_of_the_kinds_whose_call_is_never_flagged(name):
    """The cut (module docstring): no call of this circuit is flagged, so every host call with k <= 4096 enqueues the short chain."""
    pal = cc.palette(name)
    quiet = pal.quiet_kinds()
    assert len(quiet) == {"L": 14, "T": 4}[name] and any(kd.op == "search" and kd.k <= 4096 for kd in quiet)
    with _shard(pal) as shard:
        _walk(pal, quiet, lambda kd, step: _host_call(shard, kd), "short-chain circuit")


@pytest.mark.parametrize("name", ["L", "T"])
def test_device_circuit_fills_poisoned_buffers_as_on_a_fresh_index(name):
    import torch
    pal = cc.palette(name)
    with _shard(pal) as shard:
        calls, stream = _DeviceCalls(pal, shard), torch.cuda.Stream()
        _walk(pal, pal.kinds, lambda kd, step: calls(kd, stream), "device circuit")


def test_two_streams_answer_does_not_depend_on_the_previous_calls_workspace():
    import torch
    pal = cc.palette("L")
    with _shard(pal) as shard:
        calls, streams = _DeviceCalls(pal, shard), (torch.cuda.Stream(), torch.cuda.Stream())

        def call(kd, step):
            out = calls(kd, streams[step % 2])
            torch.cuda.synchronize()
            return out
        _walk(pal, pal.kinds, call, "two streams")
