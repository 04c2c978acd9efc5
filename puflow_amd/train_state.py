"""Runtime state of the training step's autograd wiring (train_perop, train_fusedfn, train_ops import it, never the reverse):
the per-(device, stream) buffer caches, the capture guard, the SyncBN callback, the weight-gradient stream, and the per-call state
that `train_ops.forward_train` sets and the autograd nodes read - in their backward too.  No autograd node lives here.
Other modules read the per-call scalars when they run (deterministic()) and set them through begin_forward / end_forward: a
`from .train_state import _DET` would freeze the import-time value."""
from __future__ import annotations

import contextlib
import contextvars
import ctypes
import sys

import torch
from torch import Tensor

from . import _lib

# the caches, one entry per (device, stream) (_SIDE: per (device, k)); each keeps its own dict - the tests and check_persist_status
# index them by name, and train_ops re-exports them: the same objects behind both names
_WS, _STAT, _SYNCW, _SYNC_SUMS, _COUNTER, _DESC_BUF, _SIDE = {}, {}, {}, {}, {}, {}, {}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ws(dev, n: int) -> Tensor:
    """Grow-only fp32 scratch per (device, stream): reuse is stream-ordered - every kernel that uses it is enqueued
    on that stream before the next one overwrites it - so two streams never share a buffer."""
    key = (dev, _stream())
    t = _WS.get(key)
    if t is None or t.numel() < n:
        t = torch.empty(max(n, 1 << 20), dtype=torch.float32, device=dev)
        _WS[key] = t
    return t


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _per_stream(cache: dict, dev, make) -> Tensor:
    """cache[(device, current stream)], made by `make()` on first use: the one look-up behind _stat, _sync_words, _sync_sums,
    _counter and _desc_buf."""
    key = (dev, _stream())
    t = cache.get(key)
    if t is None:
        t = cache[key] = make()
    return t


def _zeros_kept(n: int, dtype, dev) -> Tensor:
    """Zero-initialised device words that the kernels keep zero themselves (barrier words, statistics accumulators) or that are
    STICKY across launches (the time-out word).  They must exist before a hipGraph capture starts: a `torch.zeros` inside a
    capture becomes a memset node that clears them on every replay - a time-out recorded by replay i would be erased by replay
    i + 1 before the host ever looked.  GraphedTrainStep warms up on its capture stream, so the (device, stream) entries are
    there; anything else that captures these kernels must run them once eagerly on the capture stream first."""
    if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("puflow_amd.train_state: the zero-initialised scratch words of the fused training kernels would be allocated "
                           "inside a hipGraph capture (a memset node would clear the sticky status word on every replay): run the "
                           "step once eagerly on the capture stream before capturing it (train_graph.GraphedTrainStep does)")
    return torch.zeros(n, dtype=dtype, device=dev)


def _stat(dev) -> Tensor:
    """PF_TRAIN_STAT_DOUBLES doubles per (device, stream): the column-statistics accumulators of the fused training kernels."""
    return _per_stream(_STAT, dev, lambda: _zeros_kept(_lib.PF_TRAIN_STAT_DOUBLES, torch.float64, dev))


def _sync_words(dev) -> Tensor:
    """4 zero-initialised 32-bit words per (device, stream): arrivals / generation / exits of the persistent kernels' grid
    barriers (left zero by every launch) and a sticky status word (check_persist_status)."""
    return _per_stream(_SYNCW, dev, lambda: _zeros_kept(4, torch.int32, dev))


def check_persist_status(device=None) -> None:
    """Raise if a grid barrier of a persistent training kernel timed out since the last check (its workgroups were not all
    resident: another barrier kernel or another process held the CUs).  The unit's output was NaN, the optimizer skipped the
    update on the device; the statistics accumulators of that stream are cleared here.  One word read per stream that used a
    persistent kernel: call where the host synchronises anyway."""
    for (dev, stream), t in list(_SYNCW.items()):
        if device is not None and torch.device(device) != dev:
            continue
        if int(t[3].item()):
            t.zero_()
            st = _STAT.get((dev, stream))
            if st is not None:
                st.zero_()
            raise _lib.PuflowHipError("a persistent training kernel timed out on a grid barrier (workgroups not co-resident - is the GPU "
                                      "shared with another process, or did two barrier kernels run side by side?).  Set "
                                      "net.train_persistent = False (cfg.persistent_kernels = False) on a shared device")


# ---- SyncBN on the fused kernels: the library leaves a BatchNorm layer's LOCAL column sums in `sync_sums` and calls back;
# the callback all-reduces them (stream-ordered on torch's current stream, which is the stream the kernels were enqueued on)
_SYNC_CB_T = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p)


def _sync_sums(dev) -> Tensor:
    return _per_stream(_SYNC_SUMS, dev, lambda: _zeros_kept(2 * 128 + 1, torch.float64, dev))


def _sync_cb_impl(user, sums, n, stream):
    try:
        import torch.distributed as dist
        for t in _SYNC_SUMS.values():
            if t.data_ptr() == sums:
                dist.all_reduce(t)                      # SUM over the ranks: 2 x 128 column sums + the row count
                return 0
        return 1
    except Exception as ex:                             # an exception must not unwind through the C caller
        print(f"puflow_amd: SyncBN all-reduce failed: {type(ex).__name__}: {ex}", file=sys.stderr)
        return 2


_SYNC_CB = _SYNC_CB_T(_sync_cb_impl)                    # module-level: must outlive every call


def _attach_sync(d, dev) -> None:
    """Global-batch BatchNorm statistics for a fused-kernel call (PfEcTrain / PfBnMlpTrain)."""
    d.sync_cb = ctypes.cast(_SYNC_CB, ctypes.c_void_p)
    d.sync_user = None
    d.sync_sums = _sync_sums(dev).data_ptr()


# BatchNorm statistics over all ranks: an ARGUMENT of the forward, not process state - `forward_train` takes it from the
# module (`PointInterpFlow.sync_batchnorm`, set from `cfg.sync_batchnorm`) and holds it in this context variable for the
# duration of that call; `sync_bn(True)` is the same scope for callers of the single ops (tests)
_SYNC_BN: contextvars.ContextVar = contextvars.ContextVar("puflow_sync_bn", default=False)


@contextlib.contextmanager
def sync_bn(on: bool):
    tok = _SYNC_BN.set(bool(on))
    try:
        yield
    finally:
        _SYNC_BN.reset(tok)


# Bit-reproducible training steps (debugging switch; VERDICT / ADVICE r4): `net.deterministic = True` (TrainerModule:
# `cfg.deterministic`).  forward_train copies it here at the start of every train-mode forward and the autograd functions read it
# when they run (the backward of that forward included): BatchNorm statistics as exact 64-bit fixed-point sums
# (PF_TRAIN_DETERMINISTIC: csrc/pf_train_stat.h stat_add; the persistent kernels are not used), the latent's gradient as a gather
# over the sorted transposed neighbour lists, the Chamfer gradient by pf_chamfer_bwd_det.  Everything else in the fused step is
# already order-fixed (split-K partials reduced in index order, the dQ gather over the now sorted lists, the auction).
_DET = False


def set_deterministic(on: bool) -> None:
    global _DET
    _DET = bool(on)


def deterministic() -> bool:
    return _DET


# Weight gradients beside the backward chain (csrc/api.hip pf_train_set_dw_stream) - an opt-in that did NOT pay at the bench
# shape.  The backward of a unit produces the gradient of its input - which the unit before it waits for - and the gradients of
# its weights, which nothing reads before the optimizer: with the switch on (`net.train_dw_stream = True` / cfg.dw_stream)
# the split-K weight-gradient kernels and their reductions of the EdgeConv units and the
# conditioner / merge MLPs go to one more stream (a third parallel branch of the captured step), ~0.9 ms of the main chain's
# ~3.9 ms of kernels at 32 x (256 -> 1024).  Their workspaces come from that stream's own pool, every buffer they read is kept
# alive until the join, and the join - the calling stream waits for the weight-gradient stream - is an autograd end-of-pass
# callback, queued by the first backward function that uses the stream: whoever reads `.grad` after `backward()` sees finished
# gradients, eager or captured.  Same kernels, same arithmetic, same bits (tests/test_gpu_train.py).  Measured, same box, two
# rounds each: 4.54 -> 4.79 ms per captured step with the persistent EdgeConv kernels, 5.22 -> 5.31 without - the step is bound
# by the SUM of its kernels' work (each of them fills the chip), not by the length of the dependent chain, and kernels that share
# the chip slow each other down by more than the chain gets shorter.  (The flow chains stay on the calling stream in any case:
# f and g share their parameters, so autograd adds their gradients there before any join.)
_DW_NET = False
_DW_STREAMS = {}
_DW_PASS = {"pending": False, "keep": [], "streams": []}


def _dw_join() -> None:
    """End of the autograd pass (calling thread): the consumer of the gradients waits for the weight-gradient stream."""
    for st in _DW_PASS["streams"]:
        torch.cuda.current_stream(st.device).wait_stream(st)
    _DW_PASS["pending"] = False
    _DW_PASS["keep"] = []
    _DW_PASS["streams"] = []


def _dw_begin(dev, *keep):
    """The weight-gradient stream for one backward call on `dev`, or None (switch off, SyncBN, not inside an autograd pass).
    `keep`: tensors the side kernels read - held until the join so that the allocator cannot hand their memory to the main chain."""
    if not _DW_NET or _sync_bn_active():
        return None
    # one join per autograd pass, keyed by the pass's id: a pass that died with an exception must not leave the next one without
    tid = torch._C._current_graph_task_id() if hasattr(torch._C, "_current_graph_task_id") else 0
    if tid < 0:
        return None                                        # a backward function called by hand, outside an autograd pass
    if _DW_PASS["pending"] is not True or _DW_PASS.get("task") != tid:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_dw_join)
        except RuntimeError:
            return None
        if _DW_PASS.get("task") != tid:                    # leftovers of a pass that never reached its join
            _DW_PASS["keep"], _DW_PASS["streams"] = [], []
        _DW_PASS["pending"], _DW_PASS["task"] = True, tid
    st = _DW_STREAMS.get(dev)
    if st is None:
        st = _DW_STREAMS[dev] = torch.cuda.Stream(device=dev)
    if st not in _DW_PASS["streams"]:
        _DW_PASS["streams"].append(st)
    _DW_PASS["keep"].append(keep)
    return st


def _dw_ws(st, dev, n: int) -> Tensor:
    """_ws of the weight-gradient stream `st` (None: of the current stream)."""
    if st is None:
        return _ws(dev, n)
    with torch.cuda.stream(st):
        return _ws(dev, n)


@contextlib.contextmanager
def _dw_call(st):
    """`with _dw_call(st):` around ONE backward entry point: the library's weight-gradient stream is a per-thread setting (the
    autograd engine runs backward functions on its own device threads), set for exactly that call."""
    if st is not None:
        _lib.load().pf_train_set_dw_stream(st.cuda_stream)
    try:
        yield
    finally:
        if st is not None:
            _lib.load().pf_train_set_dw_stream(None)


def _multi_rank() -> bool:
    from .dist import multi_rank
    return multi_rank()


def _sync_bn_active() -> bool:
    return bool(_SYNC_BN.get()) and _multi_rank()


def _counter(dev) -> Tensor:
    """One zero-initialised 32-bit word per (device, stream): the arrival counter of the in-kernel grid reductions (reset by
    the workgroup that uses it last)."""
    return _per_stream(_COUNTER, dev, lambda: torch.zeros(1, dtype=torch.int32, device=dev))


_FC_IMG = {}                     # device -> (key, image) of the last flow-chain forward (FlowChainFn.forward)
_FC_SCOPE = [0, 0]               # [id of the forward_train call in progress (0: none), calls so far]
_NBT_PENDING = None        # inside forward_train: the BatchNorm layers whose batch counters are bumped by ONE launch at its end


def _count_batches(bns) -> None:
    """num_batches_tracked += 1 (torch.nn.BatchNorm in train mode): deferred to the end of the training forward when one is
    running (a launch per unit is pure latency on the step's dependency chain), immediate otherwise."""
    if _NBT_PENDING is not None:
        _NBT_PENDING.extend(bns)
        return
    with torch.no_grad():
        torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)


def begin_forward(det: bool, dw_stream: bool) -> None:
    """The per-call state of one `forward_train`: set here, read by the nodes of that forward and of its backward."""
    global _NBT_PENDING, _DW_NET
    _NBT_PENDING = []
    set_deterministic(det)
    _DW_NET = bool(dw_stream)
    _FC_SCOPE[1] += 1
    _FC_SCOPE[0] = _FC_SCOPE[1]


def end_forward() -> None:
    global _NBT_PENDING
    _FC_SCOPE[0] = 0
    _FC_IMG.clear()
    pending, _NBT_PENDING = _NBT_PENDING, None
    if pending:                                   # on the calling stream, after the side stream has been joined
        _count_batches(pending)


def _side_stream(dev, k: int = 0) -> "torch.cuda.Stream":
    st = _SIDE.get((dev, k))
    if st is None:
        st = _SIDE[(dev, k)] = torch.cuda.Stream(device=dev)
    return st


def _desc_buf(dev) -> Tensor:
    return _per_stream(_DESC_BUF, dev, lambda: torch.empty(16 * ctypes.sizeof(_lib.PfMlpTrain), dtype=torch.uint8, device=dev))
