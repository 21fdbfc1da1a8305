"""The stream layer of the model path: the side streams and every fork, join and wait between streams that
``update.py`` and ``foundation_stereo.py`` issue (``ops.py``'s pack cache and ``dist.py`` keep their own)."""
from __future__ import annotations

import contextlib

import torch

from . import ops

# Side streams per device, by slot -- who runs where:
#   MOTION   0  context net (+ stem_2, CAM / SAM) before the loop; the motion path (lookup + encoder) in the
#               loop; the mask head in the last iteration of run_pipelined
#   BRANCH   1  FeatureAtt gates; the hourglass's disparity-transformer branch; the SelectiveConvGRU small
#               branch; the mask head of forward_overlapped
#   PIPELINE 3  gru16 / gru08 one iteration ahead (run_pipelined)
# A caller forks work with ``with fork(side, origin):`` and takes it back with ``join(origin, side, *tensors)``;
# ``on(stream)`` enqueues behind what the stream already holds, without a wait.  Whether work leaves the origin is
# the caller's choice of ``side``: a call site writes its sequence once, forked, and passes the origin itself as
# the side stream to run it in order (update.OVERLAP or PIPE_BRANCH off, MOTION_ON_MAIN): fork and join then do nothing.
MOTION, BRANCH, PIPELINE = 0, 1, 3
NAMES = {MOTION: "motion", BRANCH: "branch", PIPELINE: "pipeline"}

_SIDE = {}


def side(device, slot):
    """Side stream ``slot`` (MOTION / BRANCH / PIPELINE) of ``device``."""
    s = _SIDE.get((device, slot))
    if s is None:
        # all at default priority: ANY side stream at high priority -- motion (round 4), the branch or
        # the pipeline stream (round 5) -- measured 14.5-14.7 vs 19.0-20.9 pairs/s
        s = _SIDE[(device, slot)] = torch.cuda.Stream(device=device)
    return s


def current(device):
    return torch.cuda.current_stream(device)


def capturing() -> bool:
    return torch.cuda.is_current_stream_capturing()


def capture_id(device):
    """Id of the hipGraph capture the current stream of ``device`` is part of; None outside capture."""
    return ops.stream_capture_id(current(device).cuda_stream) if capturing() else None


def on(stream):
    """Context: ``stream`` is the current stream."""
    return torch.cuda.stream(stream)


def record(stream):
    """An event after the work enqueued on ``stream`` so far (``join(..., event=)`` waits for that only)."""
    return stream.record_event()


def keep(t, stream):
    """``t`` (allocated on another stream) is in use on ``stream``: not recycled before that work is done."""
    t.record_stream(stream)


# capture_fork -- the rule every fork / join of a side stream here follows under hipGraph capture:
# a side stream waits only on the capture's origin stream (or on a stream that never waits on it in
# turn); it may be waited on by any stream, and is joined back by the origin.  On this ROCm (HIP 7,
# torch 2.10) a side stream X that waits on side stream A which later waits on X (a fork from a side
# stream plus its join) makes hipStreamEndCapture segfault: tools/capture_fork_probe.py reproduces it
# with plain torch ops (variants a_only, two_parents, enter_main_wait_side segfault; main_only,
# via_main pass).  Hence gru08's small branch on the pipeline stream runs in order, and the motion
# path's disparity branch forks from main, not from the motion stream.
#
# Enforced by ``wait`` (every wait between streams of the model path goes through it): while a capture is
# in progress it records the waits between side streams and raises before a wait that would close a cycle
# (X waiting on A after A waited on X, directly or through other side streams) -- every variant the
# probe saw segfault has such a mutual wait, every variant that passed has none.  The recorded waits
# belong to one capture, identified by its id (hipStreamGetCaptureInfo): a new id drops the old ones.
_CAPTURE_EDGES = {}          # capture id -> {key(waiter): set of key(waited)}, side streams only; one id at a time


def _skey(s):
    """A stream's identity: its HIP handle (torch.cuda.current_stream() returns a new Python wrapper on
    every call, so id() of the wrapper does not identify the stream); id() for handle-less stand-ins."""
    h = getattr(s, "cuda_stream", None)
    return ("hip", h) if h is not None else ("obj", id(s))


class CaptureForkError(RuntimeError):
    """A stream wait that would make hipStreamEndCapture segfault on this ROCm (capture_fork)."""


def capture_fork_check(waiter, waited, capture_id, side_ids=None):
    """Record ``waiter`` waiting on ``waited`` in capture ``capture_id`` (None, not capturing: nothing to record);
    raise CaptureForkError when ``waited`` already (transitively) waits on ``waiter`` in that capture.  Only
    edges between side streams (``side_ids``: their ``_skey``, default the ones ``side`` made) count."""
    if capture_id is None:
        return
    if capture_id not in _CAPTURE_EDGES:
        _CAPTURE_EDGES.clear()                   # another capture: its waits are not this one's
    edges = _CAPTURE_EDGES.setdefault(capture_id, {})
    sides = side_ids if side_ids is not None else {_skey(v) for v in _SIDE.values()}
    a, b = _skey(waiter), _skey(waited)
    if a == b or a not in sides or b not in sides:
        return
    seen, todo = set(), [b]
    while todo:                                  # does `waited` reach `waiter` through recorded waits?
        x = todo.pop()
        if x == a:
            raise CaptureForkError("capture_fork: a side stream would wait on a side stream that already waits "
                                   "on it inside this hipGraph capture (hipStreamEndCapture segfaults on this "
                                   "ROCm; tools/capture_fork_probe.py) -- fork from the capture origin instead")
        if x not in seen:
            seen.add(x)
            todo.extend(edges.get(x, ()))
    edges.setdefault(a, set()).add(b)


# diagnostics (tools/replay_timeline.py): while a list, every wait issued during a capture is logged as
# (waiter stream handle, waited stream handle, number of clocked launches captured so far), which with
# the capture-ordered clock records gives the captured graph's cross-stream edges
WAIT_LOG = None


def wait(waiter, waited, event=None):
    """``waiter`` waits for the work enqueued on ``waited`` so far -- with ``event`` (``record(waited)``) for
    the work before the event only -- with the capture_fork check while a capture is in progress."""
    cid = capture_id(waiter.device)
    capture_fork_check(waiter, waited, cid)
    if WAIT_LOG is not None and cid is not None:
        WAIT_LOG.append((waiter.cuda_stream, waited.cuda_stream, ops.timer_captured_count()))
    if event is None:
        waiter.wait_stream(waited)
    else:
        waiter.wait_event(event)


@contextlib.contextmanager
def fork(side, origin):
    """Context: ``side`` waits for ``origin`` and is the current stream; ``side`` the origin itself: in order."""
    if _skey(side) == _skey(origin):
        yield
        return
    wait(side, origin)
    with on(side):
        yield


def join(origin, side, *tensors, event=None):
    """``origin`` waits for ``side`` (up to ``event`` when given) and takes over ``tensors`` made there;
    nothing to do when ``side`` is the origin itself."""
    if _skey(side) == _skey(origin):
        return
    wait(origin, side, event)
    for t in tensors:
        keep(t, origin)
