"""CPU: the side-stream schedule of the refinement loop, checked for races without a device.

The real ``run_pipelined`` and ``forward_overlapped`` (and the real ``SelectiveConvGRU.forward``, which owns
the small-branch fork) run against fake streams: ``streams``' primitives (``side``, ``current``, ``capturing``,
``on``, ``wait``, ``keep``) are replaced by stand-ins that keep a vector clock per stream, and every kernel
wrapper the loop calls (``_conv``, ``ops.conv2d`` / ``conv2d_gate``, ``pool2x``, ``interp``, the motion encoder,
the disparity head) by a stub that logs (stream, clock, regions read, regions written) and hands back small
CPU tensors.  A value is a region of a tensor's storage, so the disparity the head writes in place into
``enc[:, nc:]`` and the next motion path reads is followed like any other.  Over the log:

  (a) every two accesses of overlapping regions, at least one a write, are ordered (happens-before): in
      particular every value is read only by work ordered after the work that produced it;
  (b) at return the caller's stream is ordered after everything enqueued on any stream;
  (c) the waits pass ``streams.capture_fork_check`` under one capture id;
  (d) every wait has the caller's stream on one side ("fork only from the origin").

Two negative controls drop one wait each and must make (a) report a race.

Every call site writes its sequence once and picks the streams; with the side stream the caller's own,
``streams.fork`` / ``join`` (the real ones run here) do nothing.  The in-order variants -- ``OVERLAP`` off, the HIP
arm of ``forward``, ``fork_small=False`` -- must log every op on the caller's stream, issue no wait, and do the
same work as the forked run: the same multiset of (op, regions read, regions written), ``dataflow``.
"""
import collections
import contextlib
import hashlib
import types

import pytest
import torch
import torch.nn as nn

from foundationstereo_amd import ops, streams
from foundationstereo_amd import update as up

NC = 3                                     # encoder output channels before the disparity channel


class FakeStream:
    device = torch.device("cpu")

    def __init__(self, name):
        self.name = name
        self.clock = {}                    # vector clock: stream name -> number of its ops ordered before here

    def __repr__(self):
        return self.name


def region(t):
    """(storage, first element, one past the last element) a tensor spans."""
    lo = t.storage_offset()
    return (t.untyped_storage().data_ptr(), lo, lo + sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1)


def overlap(a, b):
    return a[0] == b[0] and a[1] < b[2] and b[1] < a[2]


class Sched:
    """The fake stream layer plus the log of stubbed work."""

    def __init__(self, drop=None):
        self.main = FakeStream("main")
        self.sides = {}
        self.stack = [self.main]
        self.ops = []                      # (name, stream, clock snapshot, read regions, written regions)
        self.waits = []                    # (waiter, waited) in issue order, dropped ones excluded
        self.keepalive = []                # every tensor seen: no storage address is reused while logging
        self.drop = drop                   # (waiter name, waited name, occurrence): a wait not to issue
        self.seen = {}

    # -- streams' primitives
    def side(self, device, slot):
        return self.sides.setdefault(slot, FakeStream(streams.NAMES[slot]))

    def current(self, device=None):
        return self.stack[-1]

    @contextlib.contextmanager
    def on(self, stream):
        self.stack.append(stream)
        try:
            yield
        finally:
            self.stack.pop()

    def wait(self, waiter, waited, event=None):
        k = (waiter.name, waited.name)
        n = self.seen[k] = self.seen.get(k, -1) + 1
        if self.drop == k + (n,):
            return
        self.waits.append((waiter, waited))
        for s, c in waited.clock.items():
            waiter.clock[s] = max(waiter.clock.get(s, 0), c)

    # -- stubbed work
    def rec(self, name, reads=(), writes=(), shape=None):
        """One kernel on the current stream; returns a fresh tensor when ``shape`` is given (also written)."""
        s = self.current()
        s.clock[s.name] = s.clock.get(s.name, 0) + 1
        new = torch.zeros(shape) if shape is not None else None
        reads = [t for t in reads if t is not None]
        writes = list(writes) + ([new] if new is not None else [])
        self.keepalive += reads + writes
        self.ops.append((name, s, dict(s.clock), [region(t) for t in reads], [region(t) for t in writes]))
        return new

    # -- the checks
    def races(self):
        """(a): conflicting accesses not ordered by happens-before, as (earlier op, later op) names."""
        out = []
        for j, (nb, sb, cb, rb, wb) in enumerate(self.ops):
            for na, sa, ca, ra, wa in self.ops[:j]:
                if ca[sa.name] <= cb.get(sa.name, 0):          # a happens-before b
                    continue
                if any(overlap(x, y) for x in wa for y in rb + wb) or any(overlap(x, y) for x in ra for y in wb):
                    out.append((f"{na}@{sa}", f"{nb}@{sb}"))
        return out

    def check(self):
        assert self.races() == []
        for name, s, c, _, _ in self.ops:                      # (b)
            assert c[s.name] <= self.main.clock.get(s.name, 0), f"{name}@{s} not joined at return"
        assert self.stack == [self.main]
        side_ids = {streams._skey(s) for s in self.sides.values()}
        for w, d in self.waits:
            streams.capture_fork_check(w, d, ("host", id(self)), side_ids=side_ids)    # (c)
            assert self.main in (w, d), f"{w} waits on {d}"                            # (d)


def dataflow(sc):
    """The log as a multiset of (op, regions read, regions written).  A storage is named by the op that first
    wrote it and what that op read, not by its address: the same in two runs on the same inputs whatever the
    streams and the enqueue order of independent work."""
    ids, out = {}, collections.Counter()
    for name, _, _, reads, writes in sc.ops:
        r = tuple((ids.get(p, "unwritten"), lo, hi) for p, lo, hi in reads)
        for k, (p, lo, hi) in enumerate(writes):
            ids.setdefault(p, hashlib.sha1(repr((name, r, k, hi - lo)).encode()).hexdigest()[:16])
        out[(name, r, tuple((ids[p], lo, hi) for p, lo, hi in writes))] += 1
    return out


def assert_in_order(sc, forked):
    """``sc`` ran everything on the caller's stream without a wait, and did the work of ``forked``."""
    assert {s.name for _, s, _, _, _ in sc.ops} == {"main"}
    assert sc.waits == [] and sc.seen == {}
    assert sc.races() == []
    assert forked.waits and {s.name for _, s, _, _, _ in forked.ops} > {"main"}      # the control did fork
    assert dataflow(sc) == dataflow(forked)
    assert sum(dataflow(sc).values()) == len(sc.ops) == len(forked.ops)


def seg_tensors(segs):
    return [s[0] if isinstance(s, tuple) else s for s in segs]


@pytest.fixture
def sched(monkeypatch):
    def make(drop=None, **knobs):
        sc = Sched(drop)
        for name in ("side", "current", "on", "wait"):
            monkeypatch.setattr(streams, name, getattr(sc, name))
        monkeypatch.setattr(streams, "capturing", lambda: False)
        monkeypatch.setattr(streams, "keep", lambda t, stream: None)

        def conv2d(segs, pk, bias=None, act=None, res=None, **kw):
            ts = seg_tensors(segs)
            return sc.rec("conv2d", ts + [res], shape=ts[0].shape)

        def conv2d_gate(segs, pk, b, mode, h=None, z=None, rh=None, att=None, out=None):
            ts = seg_tensors(segs)
            if mode == "zr":
                sc.rec("gate_zr", ts + [h], [z, rh])
            else:                          # blend_large adds into what blend_small wrote
                sc.rec(mode, ts + [h, z, att] + ([out] if mode == "blend_large" else []), [out])

        monkeypatch.setattr(ops, "conv2d", conv2d)
        monkeypatch.setattr(ops, "conv2d_gate", conv2d_gate)
        monkeypatch.setattr(up, "_conv", lambda mods, segs, act=None, **kw: conv2d(segs, None, act=act, **kw))
        monkeypatch.setattr(up, "_packed", lambda *mods, cin_order=None: (None, None))
        monkeypatch.setattr(up, "_fast", lambda x: True)
        monkeypatch.setattr(up, "pool2x", lambda x: sc.rec("pool2x", [x], shape=x.shape))
        monkeypatch.setattr(up, "interp", lambda x, dest: sc.rec("interp", [x], shape=dest.shape))
        monkeypatch.setattr(up, "OVERLAP", True)
        for k, v in knobs.items():
            monkeypatch.setattr(up, k, v)
        return sc
    return make


def make_block(sc, n_gru_layers):
    """A BasicSelectiveMultiUpdateBlock without weights: real schedule code, stubbed kernels."""
    def gru():
        g = up.SelectiveConvGRU.__new__(up.SelectiveConvGRU)
        nn.Module.__init__(g)
        g.__dict__.update(conv0=[None], conv1=[None], small_gru=types.SimpleNamespace(convz=1, convr=1, convq=1),
                          large_gru=types.SimpleNamespace(convz=2, convr=2, convq=2))
        return g

    def motion_into(disp, geo_fn, out):
        geo = geo_fn(disp) if geo_fn is not None else sc.rec("lookup", [disp], shape=disp.shape)
        tail = out[:, NC:]
        sc.rec("encoder", [geo, disp], [out[:, :NC]] + ([tail] if tail.data_ptr() != disp.data_ptr() else []))
        return out

    def disp_head(x, res=None, out=None, co0=0):
        if out is not None:
            sc.rec("disp_head", [x, res], [out[:, co0:co0 + 1]])
            return out
        return sc.rec("disp_head", [x, res], shape=(1, 1) + tuple(x.shape[2:]))

    blk = up.BasicSelectiveMultiUpdateBlock.__new__(up.BasicSelectiveMultiUpdateBlock)
    nn.Module.__init__(blk)
    blk.__dict__.update(args=types.SimpleNamespace(n_gru_layers=n_gru_layers), mask=[None] * 4, disp_head=disp_head,
                        encoder=types.SimpleNamespace(conv=types.SimpleNamespace(out_channels=NC),
                                                      motion_into=motion_into),
                        gru04=gru(), gru08=gru(), gru16=gru() if n_gru_layers == 3 else None)
    return blk


def inputs(sc, levels=3):
    """net, inp, att, pre per level (sizes 4, 2, 1) and the initial disparity, produced on the caller's stream."""
    def lvl(name):
        return [sc.rec(name, shape=(1, 2, 4 >> i, 4 >> i)) for i in range(levels)]
    return lvl("net"), lvl("inp"), lvl("att"), lvl("pre"), sc.rec("init_disp", shape=(1, 1, 4, 4))


def run_pipelined(sc, iters):
    blk = make_block(sc, 3)
    net, inp, att, pre, disp = inputs(sc)
    net, mask, disp = blk.run_pipelined(net, inp, None, disp, att, iters, pre=pre)
    sc.rec("upsample", [disp, mask, *net])                  # the caller reads every result on its stream
    return sc


@pytest.mark.parametrize("motion_on_main", [False, True])
@pytest.mark.parametrize("pipe_branch", [True, False])
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_run_pipelined(sched, iters, pipe_branch, motion_on_main):
    sc = run_pipelined(sched(PIPE_BRANCH=pipe_branch, MOTION_ON_MAIN=motion_on_main), iters)
    sc.check()
    # the motion stream always runs the last iteration's mask head
    used = {s.name for _, s, _, _, _ in sc.ops}
    assert used == {"main", "pipeline", "motion"} | ({"branch"} if pipe_branch else set())
    assert sum(n == "lookup" and s.name == "motion" for n, s, _, _, _ in sc.ops) == (0 if motion_on_main else iters)
    # the small branch forks to the branch stream from gru04 only: once per iteration
    assert sum(n == "blend_small" and s.name == "branch" for n, s, _, _, _ in sc.ops) == (iters if pipe_branch else 0)
    assert sum(n == "blend_small" and s.name == "pipeline" for n, s, _, _, _ in sc.ops) == 2 * iters


@pytest.mark.parametrize("n_gru_layers", [3, 2])
def test_forward_overlapped(sched, n_gru_layers):
    sc = sched()
    blk = make_block(sc, n_gru_layers)
    net, inp, att, _, disp = inputs(sc, n_gru_layers)
    for _ in range(2):
        net, mask, delta = blk.forward_overlapped(net, inp, None, disp, att)
        disp = sc.rec("add", [disp, delta], shape=disp.shape)
        sc.rec("upsample", [disp, mask])
    sc.check()
    assert {s.name for _, s, _, _, _ in sc.ops} == {"main", "motion", "branch"}
    assert sum(n == "blend_small" for n, _, _, _, _ in sc.ops) == 2 * n_gru_layers


def iterate(sc, n_gru_layers, hip_forward):
    """Two iterations of ``forward_overlapped``, or of ``forward``'s HIP arm on a looked-up ``corr``."""
    blk = make_block(sc, n_gru_layers)
    net, inp, att, _, disp = inputs(sc, n_gru_layers)
    for _ in range(2):
        if hip_forward:
            net, mask, delta = blk.forward(net, inp, sc.rec("lookup", [disp], shape=disp.shape), disp, att)
        else:
            net, mask, delta = blk.forward_overlapped(net, inp, None, disp, att)
        disp = sc.rec("add", [disp, delta], shape=disp.shape)
        sc.rec("upsample", [disp, mask])
    sc.check()
    return sc


@pytest.mark.parametrize("hip_forward", [False, True])
@pytest.mark.parametrize("n_gru_layers", [3, 2])
def test_iteration_in_order(sched, n_gru_layers, hip_forward):
    """``OVERLAP`` off: ``forward_overlapped`` and the HIP arm of ``forward`` run one body on the caller's stream."""
    forked = iterate(sched(), n_gru_layers, hip_forward)
    sc = iterate(sched(OVERLAP=False), n_gru_layers, hip_forward)
    assert_in_order(sc, forked)
    # forward keeps its streams to itself also with OVERLAP on: only the GRUs' small branches fork
    assert {s.name for n, s, _, _, _ in forked.ops if s.name != "main"} == (
        {"branch"} if hip_forward else {"motion", "branch"})
    assert {n for n, s, _, _, _ in forked.ops if s.name == "branch"} == (
        {"gate_zr", "blend_small"} | (set() if hip_forward else {"conv2d"}))


def test_selective_gru_fork_small(sched):
    """``fork_small=False`` (a caller on a side stream) against the forked small branch."""
    def run(sc, fork_small):
        gru = make_block(sc, 3).gru04
        (h,), (x0,), (att,), (pre,), _ = inputs(sc, 1)
        x1 = sc.rec("motion", shape=h.shape)
        out = gru(att, h, x0, x1, pre=pre, fork_small=fork_small)
        sc.rec("reader", [out])
        sc.check()
        return sc
    assert_in_order(run(sched(), False), run(sched(), True))


# negative controls: with one wait of the schedule not issued, (a) must report the race it guarded
@pytest.mark.parametrize("drop,pair", [
    # the join of the motion stream before gru04(1): gru04 reads the encoder output
    (("main", "motion", 2), ("encoder@motion", "conv2d@main")),
    # wait(pipeline, main) before gru08(1): its pool2x reads gru04(0)'s state
    (("pipeline", "main", 1), ("blend_large@main", "pool2x@pipeline")),
])
def test_checker_reports_a_dropped_wait(sched, drop, pair):
    sc = run_pipelined(sched(drop=drop, PIPE_BRANCH=True, MOTION_ON_MAIN=False), 3)
    assert sc.seen[drop[:2]] >= drop[2]                       # the wait exists in the schedule
    assert pair in sc.races()
