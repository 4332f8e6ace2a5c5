"""ParallelizedSGD -- the reference's Optimizer API and driver loop, with the per-partition
chains, the per-sample Gradient/SGDUpdater math and the model averaging on MI355X.

Reference: src/main/scala/org/apache/spark/mllib/optimization/ParallelizedSGD.scala
  class ParallelizedSGD(gradient, updater)  :41-159   -> class ParallelizedSGD below
  object ParallelizedSGD.runParallelizedSGD :188-306  -> ParallelizedSGD.runParallelizedSGD
  8-argument alias (tol 0.001)              :311-321  -> the default of convergenceTol
  isConverged                               :324-336  -> device terms + the comparison here

What runs where: the driver loop below is the reference's, statement for statement (loss
history, regVal lag, driver-side convergence test, empty-data and empty-batch rules). The block
the reference ships to executors (:238-276: broadcast, sample, mapPartitions chain, treeReduce)
is one psgd_run_epoch_device call per process (HIP chain kernel + on-device fold in partition
order), then -- with several processes -- an all-gather of the per-process partial results over
RCCL and the same fold in rank order (the cross-GPU level of the treeReduce).
"""
from __future__ import annotations

import collections
import logging
import math
import threading
import time
import uuid
from typing import List, Optional, Tuple

import numpy as np

from . import _native as N
from .data import (CsrPartition, DensePartition, DeviceCsrPartition, DevicePartition, PartitionedData,
                   shard_range)
from .gradient import (Gradient, LeastSquaresGradient, LogisticGradient, gradient_kind, num_classes,
                       weight_dim)
from .updater import AdamSGDUpdater, SGDUpdater, updater_kind

log = logging.getLogger("org.apache.spark.mllib.optimization.ParallelizedSGD")

IllegalArgumentException = N.IllegalArgumentException


def _require(cond: bool, msg: str) -> None:
    if not cond:
        raise IllegalArgumentException("requirement failed: " + msg)


def _jstr(x) -> str:
    """Scala string interpolation of a Double/Int."""
    if isinstance(x, float):
        return repr(x) if math.isfinite(x) else ("NaN" if x != x else ("Infinity" if x > 0 else "-Infinity"))
    return str(x)


def make_params(gradient, updater, stepSize, regParam, miniBatchFraction, convergenceTol,
                compute_dtype="f64", iteration=1) -> N.psgd_params:
    p = N.psgd_params()
    p.gradient = gradient_kind(gradient)
    p.num_classes = num_classes(gradient)
    p.updater = updater_kind(updater)
    p.compute_dtype = {"f64": N.F64, "f32": N.F32}[compute_dtype]
    p.iteration = iteration
    p.step_size = float(stepSize)
    p.reg_param = float(regParam)
    p.mini_batch_fraction = float(miniBatchFraction)
    p.convergence_tol = float(convergenceTol)
    if isinstance(updater, AdamSGDUpdater):
        p.adam_beta, p.adam_gamma, p.adam_eps = updater.beta, updater.gamma, updater.eps
    else:
        p.adam_beta, p.adam_gamma, p.adam_eps = 0.9, 0.999, 1e-8
    return p


def _dist():
    """(rank, world, process_group_available) from torch.distributed, if initialised."""
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size(), True
    except ImportError:
        pass
    return 0, 1, False


# ---------------------------------------------------------------------------------------------
# Engines: who runs the chains of this process's partitions.
# ---------------------------------------------------------------------------------------------
_contexts = {}


def get_context(device: int) -> N.Context:
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = N.Context(device)
        ctx.registered_token = None
        # serialises (re-)registration + epoch of the engines that share this device's context
        ctx.engine_lock = threading.RLock()
        _contexts[device] = ctx
    return ctx


class ShardedEngine:
    """The multi-process part of an epoch, shared by every engine.

    Partition p belongs to rank floor(p * world / P) (contiguous blocks). Each rank
    folds its own chains (partition order) into a (d+3)-vector [w, regVal, lossSum, count];
    the ranks all-gather those partials and fold them in rank order with the reference's
    combiner -- a two-level treeReduce (ParallelizedSGD.scala:271-276). A rank without
    partitions contributes the fold's identity element (w_in, 0, 0, 0): an empty partition's
    result (ParallelizedSGD.scala:270 with count 0)."""

    def __init__(self, data: PartitionedData, rank: int, world: int, weight_dim: Optional[int] = None):
        # length of the weight vector: num_features, (K-1)*num_features for multinomial Logistic
        self.d = int(weight_dim) if weight_dim else data.num_features
        self.rank, self.world = rank, world
        self.lo, self.hi = shard_range(data.num_partitions, rank, world)
        self.n_local = self.hi - self.lo

    # subclass hooks: local_partial(params, w, with_counts) -> (partial[d+3], counts | None);
    # empty_partial(w) -> partial; fold_partials(gathered[world*(d+3)]) -> partial;
    # gather_buffer() -> tensor[world*(d+3)]
    def epoch(self, params, w, with_counts: bool = False):
        """ParallelizedSGD.scala:238-276 over all ranks: the folded [w_avg, regVal, lossSum,
        count] and (optionally) this rank's chain counts."""
        if self.n_local > 0:
            partial, counts = self.local_partial(params, w, with_counts)
        else:
            partial, counts = self.empty_partial(w), None
        if self.world == 1:
            return partial, counts
        return self.exchange(partial), counts

    def exchange(self, partial):
        """The cross-process level of the treeReduce: all-gather every rank's (d+3) partial
        (RCCL over xGMI with the nccl backend; gloo's list form on CPU) and fold them in rank
        order with the reference's combiner (ParallelizedSGD.scala:271-276)."""
        import torch.distributed as dist
        out = self.gather_buffer()
        if dist.get_backend() == "gloo":
            dist.all_gather(list(out.view(self.world, self.d + 3).unbind(0)), partial)
        else:
            dist.all_gather_into_tensor(out, partial)
        return self.fold_partials(out)


class HipEngine(ShardedEngine):
    """Runs this process's chains on one MI355X through the psgd C ABI.

    Weights and the (d+3)-double partial results stay in HBM (torch tensors serve as device
    allocations and as the RCCL all-gather buffers); every kernel and copy runs on
    `self.stream`."""

    def __init__(self, data: PartitionedData, rank: int = 0, world: int = 1,
                 device: Optional[int] = None, weight_dim: Optional[int] = None):
        import torch
        if not torch.cuda.is_available():
            raise N.DeviceError("HipEngine needs a visible MI355X (torch.cuda.is_available() is False)")
        super().__init__(data, rank, world, weight_dim)
        if device is None:
            device = torch.cuda.current_device()
        self.torch = torch
        self.device = device
        self.dev = torch.device("cuda", device)
        self.ctx = get_context(device)
        # a real stream handle: NULL would select the library's own stream
        self.stream = torch.cuda.Stream(device=self.dev)
        # two of each result buffer, alternating by epoch: an epoch's folded weights stay intact
        # while the next epoch, which reads them, runs (adopt_view)
        self._partials = [torch.empty(self.d + 3, dtype=torch.float64, device=self.dev) for _ in range(2)]
        self._folds = [torch.empty(self.d + 3, dtype=torch.float64, device=self.dev) for _ in range(2)]
        self._slot = 0
        self._partial, self._folded = self._partials[0], self._folds[0]
        self._gather = torch.empty(self.world * (self.d + 3), dtype=torch.float64, device=self.dev)
        self._counts = torch.empty(max(self.n_local, 1), dtype=torch.int64, device=self.dev)
        self._data = data
        with self.ctx.engine_lock:
            self._register(data)

    def _register(self, data: PartitionedData):
        """Register partitions [lo, hi) with the device context unless they are what it holds
        (ctx.engine_lock held). Engines on one device share its context; the key records whose
        partitions it holds."""
        token = getattr(data, "_psgd_token", None)
        if token is None:
            token = uuid.uuid4().hex
            data._psgd_token = token
        key = (token, self.lo, self.hi)
        self._key = key
        if self.ctx.registered_token == key:
            return
        self.ctx.clear()
        self.ctx.registered_token = None
        for p in range(self.lo, self.hi):
            part = data.partitions[p]
            if isinstance(part, DensePartition):
                self.ctx.register_dense(p, part.labels, part.x)
            elif isinstance(part, CsrPartition):
                self.ctx.register_csr(p, part.labels, part.row_ptr, part.col, part.val, part.d)
            elif isinstance(part, DevicePartition):
                dt = N.F32 if part.x.dtype == self.torch.float32 else N.F64
                self.ctx.register_dense_device(p, part.n_rows, part.d, int(part.x.stride(0)),
                                               part.labels.data_ptr(), part.x.data_ptr(), dt)
            elif isinstance(part, DeviceCsrPartition):
                dt = N.F32 if part.val.dtype == self.torch.float32 else N.F64
                self.ctx.register_csr_device(p, part.n_rows, part.d, part.labels.data_ptr(),
                                             part.row_ptr.data_ptr(), part.col.data_ptr(),
                                             part.val.data_ptr(), dt)
            else:
                raise IllegalArgumentException(f"unsupported partition type {type(part).__name__}")
        self._apply_column_transform(data)
        self.ctx.registered_token = key

    def _apply_column_transform(self, data: PartitionedData):
        """The data set's StandardScalerModel.transform, if it carries one: scales the context's
        fresh copy of the rows in place (psgd_transform_columns_device on self.stream), once per
        registration -- the token is set only afterwards, so no epoch or scoring call of any engine
        sees unscaled rows (ctx.engine_lock held)."""
        tr = getattr(data, "column_transform", None)
        if tr is None or self.n_local == 0:
            return
        shift, factor = tr
        torch = self.torch
        with torch.cuda.stream(self.stream):
            f = torch.from_numpy(np.ascontiguousarray(factor, dtype=np.float64)).to(self.dev)
            s = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift, dtype=np.float64)).to(self.dev)
            self.ctx.transform_columns_device(None if s is None else s.data_ptr(), f.data_ptr(),
                                              self.stream.cuda_stream)
        self.stream.synchronize()   # f and s are temporaries of this call

    # driver hooks ---------------------------------------------------------------------------
    def weights(self, w_host: np.ndarray):
        with self.torch.cuda.stream(self.stream):
            return self.torch.from_numpy(np.ascontiguousarray(w_host, dtype=np.float64)).to(self.dev)

    def initial_regval(self, params, w_host: np.ndarray) -> float:
        return self.ctx.initial_regval(params, w_host)

    def epoch(self, params, w_dev, with_counts: bool = False):
        """The folded partial is written on `self.stream`. Its readers may be on any stream: the
        caller's current stream is made to wait for the epoch before this returns, so a read
        there (e.g. `.cpu()` on the default stream) sees the finished result -- never the
        buffer's previous contents, which the driver would take for an empty batch (count 0,
        ParallelizedSGD.scala:295-297)."""
        caller = self.torch.cuda.current_stream(self.dev)
        # order after whatever produced the inputs on the caller's stream
        self.stream.wait_stream(caller)
        out = self._enqueue(params, w_dev, with_counts)
        caller.wait_stream(self.stream)
        return out

    def _enqueue(self, params, w_dev, with_counts=False):
        """The epoch on self.stream (into the next pair of result buffers), no cross-stream order."""
        self._slot ^= 1
        self._partial, self._folded = self._partials[self._slot], self._folds[self._slot]
        with self.torch.cuda.stream(self.stream):
            return super().epoch(params, w_dev, with_counts)

    def local_partial(self, params, w_dev, with_counts):
        # The lock serialises re-registration and the enqueue; the device order of epochs that
        # share the context's scratch buffers from different streams is the library's
        # (psgd_run_epoch_device waits for the previous epoch's end event on another stream).
        with self.ctx.engine_lock:
            # another engine on this device may have registered its own partitions since
            if self.ctx.registered_token != self._key:
                self._register(self._data)
            counts_ptr = self._counts.data_ptr() if with_counts else None
            if self._mirror_next is not None and self.world == 1:
                self.ctx.run_epoch_device_mirror(params, w_dev.data_ptr(), self._partial.data_ptr(), counts_ptr,
                                                 self.stream.cuda_stream, self._mirror_next)
                self._mirror_used = True
            else:
                self.ctx.run_epoch_device(params, w_dev.data_ptr(), self._partial.data_ptr(), counts_ptr,
                                          self.stream.cuda_stream)
        counts = self._counts[: self.n_local].cpu().numpy() if with_counts else None
        return self._partial, counts

    def empty_partial(self, w_dev):
        self._partial[: self.d].copy_(w_dev)
        self._partial[self.d:].zero_()
        return self._partial

    def gather_buffer(self):
        return self._gather

    # (diagnostics) when a list, every cross-process exchange appends a pair of HIP events recorded
    # around it on self.stream: the all-gather plus the rank-order fold (bench.py times them)
    exchange_events = None

    def exchange(self, partial):
        if self.exchange_events is None:
            return super().exchange(partial)
        a = self.torch.cuda.Event(enable_timing=True)
        b = self.torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        out = super().exchange(partial)
        b.record(self.stream)
        self.exchange_events.append((a, b))
        return out

    def fold_partials(self, gathered):
        if self._mirror_next is not None:
            self.ctx.fold_partials_device_mirror(self.world, self.d, gathered.data_ptr(), self._folded.data_ptr(),
                                                 self.stream.cuda_stream, self._mirror_next)
            self._mirror_used = True
        else:
            self.ctx.fold_partials_device(self.world, self.d, gathered.data_ptr(),
                                          self._folded.data_ptr(), self.stream.cuda_stream)
        return self._folded

    def scalars(self, folded) -> Tuple[float, float, int]:
        with self.torch.cuda.stream(self.stream):
            h = folded[self.d:].cpu().numpy()
        if not math.isfinite(h[2]):
            raise N.DeviceError("chain kernel watchdog fired (loader/compute waves stalled)")
        return float(h[0]), float(h[1]), int(h[2])

    def adopt(self, folded):
        with self.torch.cuda.stream(self.stream):
            return folded[: self.d].clone()

    # the driver's pipelined loop (ParallelizedSGD._run_pipelined) ------------------------------
    # An epoch's three scalars reach the host without a copy: the epoch's last fold kernel writes
    # them to a page-locked slot as well (psgd_run_epoch_device_mirror /
    # psgd_fold_partials_device_mirror), the count last; the host polls the count.
    _PIN_SLOTS = 16
    _mirror = None
    _mirror_next = None
    _mirror_used = False

    def epoch_async(self, params, w_dev):
        """epoch() that returns (folded, token) at once; scalars_wait(token) gives its scalars.
        Tokens are read in the order they were made, fewer than _PIN_SLOTS behind the newest.
        Unlike epoch() it orders nothing against the caller's stream (each cross-stream wait
        costs the device ~20 us between epochs): w_dev must have been produced on self.stream
        (weights(), adopt(), adopt_view() all are), and `folded` is read on self.stream or after
        scalars_wait(token)."""
        if self._mirror is None:
            self._mirror = self.ctx.host_array((self._PIN_SLOTS, 3), np.float64)
            self._pin_owner = [-1] * self._PIN_SLOTS
            self._pin_seq = 0
        seq = self._pin_seq
        k = seq % self._PIN_SLOTS
        if self._pin_owner[k] >= 0:
            self._poll(k)   # (a slot is reused only after its last epoch's fold has written it)
        self._mirror[k, 2] = self._UNSET   # the fold's count replaces it (psgd.h)
        self._mirror_next, self._mirror_used = self._mirror[k].ctypes.data, False
        try:
            folded, _ = self._enqueue(params, w_dev)
        finally:
            used, self._mirror_next = self._mirror_used, None
        if not used:   # (no fold of this epoch ran on this rank's context: copy the scalars)
            with self.torch.cuda.stream(self.stream):
                self.torch.from_numpy(self._mirror[k]).copy_(folded[self.d:])
        self._pin_owner[k] = seq
        self._pin_seq = seq + 1
        return folded, (seq, k)

    _UNSET = -1.0            # no count is negative
    _WAIT_LIMIT_S = 600.0    # a chain kernel's own watchdog ends a stalled epoch in seconds

    def scalars_wait(self, token) -> Tuple[float, float, int]:
        """scalars() of the epoch behind `token`: polls its slot until the fold kernel's count
        lands (no event: each event recorded between epochs costs the device a few us)."""
        seq, k = token
        if self._pin_owner[k] != seq:
            raise RuntimeError(f"the scalars of epoch token {seq} were overwritten before they were read")
        self._poll(k)
        h = self._mirror[k].copy()
        if not math.isfinite(h[2]):
            raise N.DeviceError("chain kernel watchdog fired (loader/compute waves stalled)")
        return float(h[0]), float(h[1]), int(h[2])

    def _poll(self, k):
        slot = self._mirror[k]
        if slot[2] != self._UNSET:
            return
        t0 = time.perf_counter()
        spins = 0
        while slot[2] == self._UNSET:
            spins += 1
            if spins > 2000:   # past the first ~ms: yield between polls
                time.sleep(20e-6)
                if time.perf_counter() - t0 > self._WAIT_LIMIT_S:
                    raise N.DeviceError("an epoch's fold did not complete")

    def drain(self):
        """Wait for everything enqueued on the engine's stream."""
        self.stream.synchronize()

    def adopt_view(self, folded):
        """adopt() without the copy: the folded weights in place, intact until the second epoch
        after the one that produced them is enqueued (the result buffers alternate)."""
        return folded[: self.d]

    def convergence_terms(self, prev, cur) -> Tuple[float, float]:
        return self.ctx.convergence_terms_device(int(cur.shape[0]), prev.data_ptr(), cur.data_ptr(),
                                                 self.stream.cuda_stream)

    def to_host(self, w_dev) -> np.ndarray:
        with self.torch.cuda.stream(self.stream):
            return w_dev.detach().cpu().numpy().astype(np.float64)

    # scoring at fixed weights (psgd_evaluate_device / psgd_predict_device) ----------------------
    def _score_weights(self, w):
        """w (host array or device tensor) as a contiguous f64 tensor on the engine's device, one
        entry per feature (self.stream is current)."""
        nf = self._data.num_features
        if self.torch.is_tensor(w):
            w_dev = w.detach().to(device=self.dev, dtype=self.torch.float64).contiguous()
        else:
            w_dev = self.torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(self.dev)
        if w_dev.dim() != 1 or w_dev.shape[0] != nf:
            raise IllegalArgumentException(
                f"requirement failed: BLAS.dot(x: Vector, y: Vector) was given Vectors with "
                f"non-matching sizes: x.size = {nf}, y.size = {w_dev.numel()}")
        return w_dev

    def evaluate(self, gradient, w) -> "EngineScore":
        """lossSum (gradient.compute(x, y, w)._2 summed), count and nCorrect of weights w over every
        partition of the data, on all ranks, with the per-partition sums (psgd_evaluate_device: one
        streaming fp64 pass, deterministic sums). w: a host array or a device tensor of
        num_features doubles. With several ranks each scores its own partitions; the ranks
        all-gather their three sums and per-partition pairs (the backends of exchange()) and add
        lossSum in rank order, which is partition order (the blocks are contiguous); a rank without
        partitions contributes zeros. Every registered row counts, whatever an earlier epoch sampled."""
        if num_classes(gradient) > 2:
            raise N.UnsupportedOperationException(
                "evaluate with the multinomial LogisticGradient (numClasses > 2) is not built: "
                "use evaluate_multinomial")
        kind = gradient_kind(gradient)
        return self._score_all(self._score_weights, w, lambda w_ptr, out3, part: self.ctx.evaluate_device(
            kind, w_ptr, out3, part, self.stream.cuda_stream))

    def _score_all(self, to_device, w, enqueue) -> "EngineScore":
        """The frame of evaluate / evaluate_multinomial: w through to_device on self.stream,
        enqueue(w_ptr, out3_ptr, part_ptr) for this rank's partitions, the ranks' all-gather and
        the sums in rank order."""
        torch = self.torch
        P = self._data.num_partitions
        shards = [shard_range(P, r, self.world) for r in range(self.world)]
        width = 3 + 2 * max(max(hi - lo for lo, hi in shards), 1)
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            w_dev = to_device(w)
            buf = torch.zeros(width, dtype=torch.float64, device=self.dev)
            if self.n_local > 0:
                with self.ctx.engine_lock:
                    if self.ctx.registered_token != self._key:
                        self._register(self._data)
                    enqueue(w_dev.data_ptr(), buf.data_ptr(), buf.data_ptr() + 24)
            if self.world > 1:
                import torch.distributed as dist
                out = torch.empty(self.world * width, dtype=torch.float64, device=self.dev)
                if dist.get_backend() == "gloo":
                    dist.all_gather(list(out.view(self.world, width).unbind(0)), buf)
                else:
                    dist.all_gather_into_tensor(out, buf)
                h = out.cpu().numpy().reshape(self.world, width)
            else:
                h = buf.cpu().numpy().reshape(1, width)
        loss_sum, count, correct = 0.0, 0, 0
        part_loss, part_correct = np.zeros(P), np.zeros(P, dtype=np.int64)
        for r, (lo, hi) in enumerate(shards):   # rank order = partition order
            loss_sum = loss_sum + float(h[r, 0])
            count += int(h[r, 1])
            correct += int(h[r, 2])
            pairs = h[r, 3: 3 + 2 * (hi - lo)].reshape(hi - lo, 2)
            part_loss[lo:hi] = pairs[:, 0]
            part_correct[lo:hi] = pairs[:, 1].astype(np.int64)
        return EngineScore(loss_sum, count, correct, part_loss, part_correct)

    def predict(self, p: int, w):
        """The raw dots x_r . w of local partition p's rows, in iterator order, as a device tensor
        (psgd_predict_device); the caller applies its own threshold or link function."""
        if not (self.lo <= p < self.hi):
            raise IllegalArgumentException(
                f"requirement failed: partition {p} is not held by rank {self.rank} "
                f"(its partitions are [{self.lo}, {self.hi}))")
        torch = self.torch
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            w_dev = self._score_weights(w)
            n = self._data.partitions[p].n_rows
            out = torch.empty(n, dtype=torch.float64, device=self.dev)
            with self.ctx.engine_lock:
                if self.ctx.registered_token != self._key:
                    self._register(self._data)
                self.ctx.predict_device(p, w_dev.data_ptr(), out.data_ptr(), self.stream.cuda_stream)
            keep = torch.cuda.Event()
            keep.record(self.stream)
        caller.wait_stream(self.stream)
        out.record_stream(caller)
        keep.synchronize()   # w_dev may be a temporary of this call
        return out

    # scoring a multinomial logistic model (psgd_evaluate_multinomial_device and its kin) ----------
    def _multinomial_weights(self, numClasses: int):
        """to_device for (K - 1) * num_features weights (MLlib's require on weights.size)."""
        nf, K = self._data.num_features, int(numClasses)

        def to_device(w):
            if self.torch.is_tensor(w):
                w_dev = w.detach().to(device=self.dev, dtype=self.torch.float64).contiguous()
            else:
                w_dev = self.torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(self.dev)
            check_multinomial_weights(K, nf, int(w_dev.numel()) if w_dev.dim() == 1 else -1)
            return w_dev
        return to_device

    def evaluate_multinomial(self, numClasses: int, w) -> "EngineScore":
        """evaluate() for LogisticGradient(numClasses = K > 2): lossSum, count and nCorrect (rows
        whose predictPoint class equals the label) of the (K - 1) * num_features weights w over
        every partition, on all ranks, with the per-partition sums
        (psgd_evaluate_multinomial_device). The same all-gather and rank-order sums as evaluate()."""
        K = check_num_classes(numClasses)
        return self._score_all(self._multinomial_weights(K), w,
                               lambda w_ptr, out3, part: self.ctx.evaluate_multinomial_device(
                                   K, w_ptr, out3, part, self.stream.cuda_stream))

    def predict_classes(self, p: int, numClasses: int, w, margins: bool = False):
        """The predicted classes of local partition p's rows as a device tensor of doubles (the
        labels' convention), in iterator order; with margins=True also the raw margins [n, K - 1]
        (psgd_predict_multinomial_device)."""
        K = check_num_classes(numClasses)
        if not (self.lo <= p < self.hi):
            raise IllegalArgumentException(
                f"requirement failed: partition {p} is not held by rank {self.rank} "
                f"(its partitions are [{self.lo}, {self.hi}))")
        torch = self.torch
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            w_dev = self._multinomial_weights(K)(w)
            n = self._data.partitions[p].n_rows
            classes = torch.empty(n, dtype=torch.float64, device=self.dev)
            m = torch.empty((n, K - 1), dtype=torch.float64, device=self.dev) if margins else None
            with self.ctx.engine_lock:
                if self.ctx.registered_token != self._key:
                    self._register(self._data)
                self.ctx.predict_multinomial_device(p, K, w_dev.data_ptr(), classes.data_ptr(),
                                                    m.data_ptr() if margins else None, self.stream.cuda_stream)
            keep = torch.cuda.Event()
            keep.record(self.stream)
        caller.wait_stream(self.stream)
        classes.record_stream(caller)
        if margins:
            m.record_stream(caller)
        keep.synchronize()   # w_dev may be a temporary of this call
        return (classes, m) if margins else classes

    def confusion(self, numClasses: int, w) -> np.ndarray:
        """The K x K confusion table (rows actual, columns predicted; int64) of weights w over every
        partition, on all ranks (psgd_confusion_model_device: the classes go to the context's scratch,
        the labels are read where the registry holds them). Several ranks all-gather their tables and
        add them: integers, exact in any order. A label that is not a whole number in [0, K) raises."""
        K = check_num_classes(numClasses)
        torch = self.torch
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            w_dev = self._multinomial_weights(K)(w)
            buf = torch.zeros(1 + K * K, dtype=torch.int64, device=self.dev)   # {n_bad, counts}
            if self.n_local > 0:
                with self.ctx.engine_lock:
                    if self.ctx.registered_token != self._key:
                        self._register(self._data)
                    self.ctx.confusion_model_device(K, w_dev.data_ptr(), buf.data_ptr() + 8, buf.data_ptr(),
                                                    self.stream.cuda_stream)
            if self.world > 1:
                import torch.distributed as dist
                out = torch.empty(self.world * (1 + K * K), dtype=torch.int64, device=self.dev)
                if dist.get_backend() == "gloo":
                    dist.all_gather(list(out.view(self.world, 1 + K * K).unbind(0)), buf)
                else:
                    dist.all_gather_into_tensor(out, buf)
                h = out.view(self.world, 1 + K * K).sum(dim=0).cpu().numpy()
            else:
                h = buf.cpu().numpy()
        if int(h[0]) > 0:
            raise IllegalArgumentException(
                f"requirement failed: {int(h[0])} labels are not whole numbers in [0, {K})")
        return h[1:].reshape(K, K).astype(np.int64)

    # binary classification metrics (psgd_binary_counts_model_device / psgd_binary_counts_device) --
    def _local_scores(self, w_dev):
        """(margins, labels) of this rank's rows in partition order, as device tensors of doubles
        (self.stream is current): psgd_predict_device per partition, the labels as the data holds them."""
        torch = self.torch
        rows = [self._data.partitions[p].n_rows for p in range(self.lo, self.hi)]
        scores = torch.empty(sum(rows), dtype=torch.float64, device=self.dev)
        labels = torch.empty(sum(rows), dtype=torch.float64, device=self.dev)
        off = 0
        with self.ctx.engine_lock:
            if self.n_local > 0 and self.ctx.registered_token != self._key:
                self._register(self._data)
            for p, n in zip(range(self.lo, self.hi), rows):
                if n == 0:
                    continue
                self.ctx.predict_device(p, w_dev.data_ptr(), scores.data_ptr() + 8 * off, self.stream.cuda_stream)
                y = self._data.partitions[p].labels
                if not torch.is_tensor(y):
                    y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64))
                labels[off: off + n].copy_(y.detach().to(device=self.dev, dtype=torch.float64))
                off += n
        return scores, labels

    def binary_counts(self, w, score: str = "margin"):
        """The BinaryClassificationMetrics table and areas of weights w over every partition of the
        data, on all ranks (evaluation.DeviceCounts; include/psgd.h has the semantics). One rank with
        score="margin": psgd_binary_counts_model_device -- the rows are scored into the context's
        scratch and their labels read where the registry holds them. score="probability" applies
        torch.sigmoid to the margins of psgd_predict_device and goes through the array form. With
        several ranks each scores its own partitions, the ranks all-gather their scores and labels
        padded to the longest (the backends of exchange()), and every rank runs the array form over
        the whole: the result does not depend on the order of the pairs, so all ranks hold the same
        bits, and the bits of one rank alone."""
        from . import evaluation as E
        if score not in ("margin", "probability"):
            raise IllegalArgumentException(f"requirement failed: score must be 'margin' or 'probability', got {score!r}")
        torch = self.torch
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            w_dev = self._score_weights(w)
            if self.world == 1 and score == "margin" and self.n_local > 0:
                n = sum(self._data.partitions[p].n_rows for p in range(self.lo, self.hi))
                thr, cp, cn, small = E.alloc_outputs(torch, self.dev, n)
                with self.ctx.engine_lock:
                    if self.ctx.registered_token != self._key:
                        self._register(self._data)
                    self.ctx.binary_counts_model_device(w_dev.data_ptr(), thr.data_ptr(), cp.data_ptr(), cn.data_ptr(),
                                                        small.data_ptr(), small.data_ptr() + 32,
                                                        self.stream.cuda_stream)
                out = E.read_outputs(thr, cp, cn, small)
            else:
                scores, labels = self._local_scores(w_dev)
                if self.world > 1:
                    import torch.distributed as dist
                    P = self._data.num_partitions
                    rows = []
                    for r in range(self.world):
                        lo, hi = shard_range(P, r, self.world)
                        rows.append(sum(self._data.partitions[p].n_rows for p in range(lo, hi)))
                    width = max(max(rows), 1)
                    buf = torch.zeros(2 * width, dtype=torch.float64, device=self.dev)
                    buf[: rows[self.rank]].copy_(scores)
                    buf[width: width + rows[self.rank]].copy_(labels)
                    got = torch.empty(self.world * 2 * width, dtype=torch.float64, device=self.dev)
                    if dist.get_backend() == "gloo":
                        dist.all_gather(list(got.view(self.world, 2 * width).unbind(0)), buf)
                    else:
                        dist.all_gather_into_tensor(got, buf)
                    got = got.view(self.world, 2, width)
                    scores = torch.cat([got[r, 0, : rows[r]] for r in range(self.world)])
                    labels = torch.cat([got[r, 1, : rows[r]] for r in range(self.world)])
                if score == "probability":
                    scores = torch.sigmoid(scores)
                out = E.counts_of_tensors(self.ctx, torch, self.stream, scores.contiguous(), labels.contiguous())
        # (the read of summary and areas has waited for self.stream: w_dev and the temporaries are free)
        caller.wait_stream(self.stream)
        for t in (out.thresholds, out.cumPos, out.cumNeg):
            t.record_stream(caller)
        return out

    # column statistics (psgd_column_stats_device) ----------------------------------------------
    def column_stats(self) -> "ColumnStats":
        """Statistics.colStats over every partition of the data, on all ranks (one streaming fp64
        pass over dense rows, two over CSR rows; include/psgd.h has the semantics). Each rank runs
        its partitions; the ranks all-gather their 1 + 5 d doubles (the backends of exchange()) and
        every rank merges them on the host in rank order with Chan's formula in fp64: counts and
        numNonzeros add, max and min are taken, a rank with count 0 is skipped. count 0 raises the
        summarizer's IllegalArgumentException."""
        torch = self.torch
        nf = self._data.num_features
        width = 1 + 5 * nf
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            buf = torch.zeros(width, dtype=torch.float64, device=self.dev)
            if self.n_local > 0:
                with self.ctx.engine_lock:
                    if self.ctx.registered_token != self._key:
                        self._register(self._data)
                    self.ctx.column_stats_device(buf.data_ptr(), self.stream.cuda_stream)
            if self.world > 1:
                import torch.distributed as dist
                out = torch.empty(self.world * width, dtype=torch.float64, device=self.dev)
                if dist.get_backend() == "gloo":
                    dist.all_gather(list(out.view(self.world, width).unbind(0)), buf)
                else:
                    dist.all_gather_into_tensor(out, buf)
                h = out.cpu().numpy().reshape(self.world, width)
            else:
                h = buf.cpu().numpy().reshape(1, width)
        return merge_column_stats(h, nf)

    # the batch gradient and the batch update (psgd_gradient_sum_device / psgd_gd_update_device) ---
    def gradient_sum(self, gradient, w, miniBatchFraction: float = 1.0, iteration: int = 0):
        """{gradientSum[d], lossSum, count} of weights w over the batch -- every row, or
        RDD.sample(false, miniBatchFraction, 42 + iteration) per partition -- on all ranks, as a device
        tensor of d + 2 doubles (include/psgd.h has the semantics). Each rank runs its partitions; the
        ranks all-gather their d + 2 doubles (the backends of exchange()) and every rank adds the rows
        in rank order (merge_gradient_sums: a loop, not a tree), so all ranks hold the same bits; a
        rank without partitions contributes zeros. w: a host array or a device tensor. The multinomial
        LogisticGradient (numClasses > 2) goes through gradient_sum_multinomial."""
        if num_classes(gradient) > 2:
            raise N.UnsupportedOperationException(
                "gradient_sum takes a binary gradient: the multinomial LogisticGradient (numClasses > 2) "
                "goes through gradient_sum_multinomial")
        kind = gradient_kind(gradient)
        return self._batch_sum(self._data.num_features + 2, self._score_weights, w,
                               lambda w_ptr, out: self.ctx.gradient_sum_device(
                                   kind, w_ptr, miniBatchFraction, iteration, out, self.stream.cuda_stream))

    def gradient_sum_multinomial(self, numClasses: int, w, miniBatchFraction: float = 1.0, iteration: int = 0):
        """gradient_sum() for LogisticGradient(numClasses = K > 2): a device tensor of
        (K - 1) * num_features + 2 doubles {gradientSum, lossSum, count} at the (K - 1) * num_features
        weights w (psgd_gradient_sum_multinomial_device). The same all-gather and rank-order sums."""
        K = check_num_classes(numClasses)
        return self._batch_sum((K - 1) * self._data.num_features + 2, self._multinomial_weights(K), w,
                               lambda w_ptr, out: self.ctx.gradient_sum_multinomial_device(
                                   K, w_ptr, miniBatchFraction, iteration, out, self.stream.cuda_stream))

    # the augmented Gramian (psgd_gramian_device / psgd_gramian_weighted_device) ------------------
    def local_rows(self) -> int:
        """The rows of this rank's partitions: the length of row_curvature()'s result and of
        gramian()'s weights."""
        return sum(self._data.partitions[p].n_rows for p in range(self.lo, self.hi))

    def gramian(self, weights=None):
        """M = sum_i z_i z_i^T with z_i = [x_i, y_i, 1] over every row of the data, on all ranks, as a
        device tensor of (d + 2)^2 doubles, row-major (include/psgd.h has the semantics; stat.Gramian
        reads it). Each rank runs its partitions; the ranks all-gather their matrices (the backends of
        exchange()) and every rank adds them in rank order (merge_gradient_sums: a loop, not a tree),
        so all ranks hold the same bits; a rank without partitions contributes zeros.
        weights: a device tensor of local_rows() doubles, one per row of this rank's partitions in
        partition and iterator order -- the result is then M_w = sum_i weights_i z_i z_i^T
        (psgd_gramian_weighted_device), the ranks' matrices added in the same way."""
        nf = self._data.num_features
        if nf > N.GRAMIAN_MAX_D:
            raise N.IllegalArgumentException(
                f"requirement failed: the Gramian takes at most {N.GRAMIAN_MAX_D} features (got {nf})")
        if weights is None:
            return self._batch_sum((nf + 2) * (nf + 2), None, None,
                                   lambda _w, out: self.ctx.gramian_device(out, self.stream.cuda_stream))
        return self._batch_sum((nf + 2) * (nf + 2), self._row_weights, weights,
                               lambda om, out: self.ctx.gramian_weighted_device(om, out, self.stream.cuda_stream))

    def device_rows(self, values):
        """A host array of local_rows() doubles as a device tensor (gramian()'s weights)."""
        with self.torch.cuda.stream(self.stream):
            t = self.torch.from_numpy(np.array(values, dtype=np.float64)).to(self.dev)   # (a copy: torch wants it writable)
        self.stream.synchronize()
        return t

    def _row_weights(self, weights):
        """weights as a contiguous f64 device tensor of local_rows() entries (self.stream is current)."""
        if not self.torch.is_tensor(weights):
            raise IllegalArgumentException(
                "requirement failed: HipEngine.gramian takes its row weights as a device tensor "
                "(stat.gramian takes a host array)")
        om = weights.detach().to(device=self.dev, dtype=self.torch.float64).contiguous()
        n = self.local_rows()
        if om.dim() != 1 or om.shape[0] != n:
            raise IllegalArgumentException(
                f"requirement failed: the weighted Gramian takes one weight per local row ({n}; got shape "
                f"{tuple(om.shape)})")
        if n == 0:   # (a valid pointer for a registry of empty partitions)
            om = self.torch.zeros(1, dtype=self.torch.float64, device=self.dev)
        return om

    # the rows' curvature (psgd_row_curvature_device) ----------------------------------------------
    def row_curvature(self, gradient, w):
        """h_i = d^2 loss / d(x_i . w)^2 of every row of this rank's partitions at weights w (a host
        array or a device tensor of num_features doubles), as a device tensor of local_rows() doubles
        in partition and iterator order: what gramian(weights=) takes to give the Hessian of the loss
        sum (include/psgd.h has the values). The rows are this rank's own, so the ranks exchange
        nothing here. HingeGradient raises UnsupportedOperationException, and so does the multinomial
        LogisticGradient (numClasses > 2)."""
        if num_classes(gradient) > 2:
            raise N.UnsupportedOperationException(
                "row_curvature takes a binary gradient: the multinomial LogisticGradient (numClasses > 2) "
                "has a matrix of curvatures per row")
        kind = gradient_kind(gradient)
        if kind == 2:   # PSGD_GRADIENT_HINGE
            raise N.UnsupportedOperationException(
                "HingeGradient has no curvature: its second derivative is 0 almost everywhere")
        return self._batch_sum(max(self.local_rows(), 1), self._score_weights, w,
                               lambda w_ptr, out: self.ctx.row_curvature_device(
                                   kind, w_ptr, out, self.stream.cuda_stream), local=True)[: self.local_rows()]

    def _batch_sum(self, width: int, to_device, w, call, local: bool = False):
        """call(w_ptr, out_ptr) over this rank's partitions into `width` zeroed doubles, then the ranks'
        all-gather and the rank-order sum (not for a `local` result, which is this rank's alone).
        to_device(w) puts the weights on the device; None for a pass that takes no weights (w_ptr is
        then None)."""
        torch = self.torch
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            w_dev = to_device(w) if to_device is not None else None
            buf = torch.zeros(width, dtype=torch.float64, device=self.dev)
            if self.n_local > 0:
                with self.ctx.engine_lock:
                    if self.ctx.registered_token != self._key:
                        self._register(self._data)
                    call(None if w_dev is None else w_dev.data_ptr(), buf.data_ptr())
            if self.world > 1 and not local:
                import torch.distributed as dist
                out = torch.empty(self.world * width, dtype=torch.float64, device=self.dev)
                if dist.get_backend() == "gloo":
                    dist.all_gather(list(out.view(self.world, width).unbind(0)), buf)
                else:
                    dist.all_gather_into_tensor(out, buf)
                buf = merge_gradient_sums(out.view(self.world, width))
            keep = torch.cuda.Event()
            keep.record(self.stream)
        caller.wait_stream(self.stream)
        buf.record_stream(caller)
        keep.synchronize()   # w_dev may be a temporary of this call
        return buf

    def batch_scalars(self, gsum) -> Tuple[float, int]:
        """(lossSum, count) of a gradient_sum result."""
        with self.torch.cuda.stream(self.stream):
            h = gsum[-2:].cpu().numpy()
        return float(h[0]), int(h[1])

    def gd_update(self, updater, w_dev, gsum, stepSize: float, iteration: int, regParam: float):
        """(w', regVal) = updater.compute(w, gradientSum / count, stepSize, iteration, regParam) on the
        device (psgd_gd_update_device); w' is a new device tensor."""
        torch = self.torch
        # order after whatever produced the inputs on the caller's stream
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.stream):
            out = torch.empty(w_dev.shape[0] + 1, dtype=torch.float64, device=self.dev)
            self.ctx.gd_update_device(updater_kind(updater), w_dev.shape[0], w_dev.data_ptr(), gsum.data_ptr(),
                                      stepSize, iteration, regParam, out.data_ptr(),
                                      out.data_ptr() + 8 * w_dev.shape[0], self.stream.cuda_stream)
            regVal = float(out[-1:].cpu().numpy()[0])
        return out[:-1], regVal


    # train/test splits (psgd_cell_select_device / psgd_gather_*_device; split.py) ------------------
    def _storage_dtype(self):
        """The torch dtype the context stores this data's rows in (f64 when it holds no partition)."""
        torch = self.torch
        for part in self._data.partitions:
            v = part.x if isinstance(part, (DensePartition, DevicePartition)) else part.val
            if torch.is_tensor(v):
                return v.dtype
            return torch.float32 if v.dtype == np.float32 else torch.float64
        return torch.float64

    def _cell_select(self, lb, ub, complement, seed, seeding):
        """cell(lb, ub, complement) over this rank's partitions (self.stream current, ctx.engine_lock
        held): (rows, offsets, counts, nnz) -- the device index array, each local partition's first
        entry in it, and the host counts after the one read-back."""
        torch = self.torch
        if self.n_local > 0 and self.ctx.registered_token != self._key:
            self._register(self._data)
        n_rows = [self._data.partitions[p].n_rows for p in range(self.lo, self.hi)]
        offs = np.concatenate([[0], np.cumsum(n_rows, dtype=np.int64)]).astype(np.int64)
        rows = torch.empty(max(int(offs[-1]), 1), dtype=torch.int32, device=self.dev)
        cn = torch.zeros(2 * max(self.n_local, 1), dtype=torch.int64, device=self.dev)
        if self.n_local > 0:
            self.ctx.cell_select_device(seed, seeding, lb, ub, complement, rows.data_ptr(), cn.data_ptr(),
                                        cn.data_ptr() + 8 * self.n_local, self.stream.cuda_stream)
        h = cn.cpu().numpy()
        return rows, offs, h[: self.n_local].copy(), h[self.n_local: 2 * self.n_local].copy()

    def cell_rows(self, lb: float, ub: float, complement: bool, seed: int, seeding: int):
        """The row indices BernoulliCellSampler(lb, ub, complement) keeps of each of this rank's
        partitions, in partition order: a list of int32 device tensors, increasing (include/psgd.h has
        the semantics; seeding is N.SEED_PLUS_INDEX for randomSplit, N.SEED_PARTITIONWISE for kFold)."""
        torch = self.torch
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            with self.ctx.engine_lock:
                rows, offs, counts, _ = self._cell_select(lb, ub, complement, seed, seeding)
            out = [rows[int(offs[i]): int(offs[i]) + int(counts[i])] for i in range(self.n_local)]
        caller.wait_stream(self.stream)
        rows.record_stream(caller)
        return out

    def split_cell(self, lb: float, ub: float, complement: bool, seed: int, seeding: int) -> PartitionedData:
        """The rows of cell(lb, ub, complement) as a PartitionedData of device partitions: the
        selection, one read-back of the counts, torch tensors for the outputs (one arena a split, the
        partitions are views of it) and one compaction launch over all partitions. It lists all P
        partitions; this rank's block is filled, empty device placeholders stand for the others';
        `partition_counts` holds every partition's row count, all-gathered, on every rank. The rows
        come from the context's registered copy: a source column_transform is in them, the result
        carries none."""
        torch = self.torch
        data, P, d = self._data, self._data.num_partitions, self._data.num_features
        csr = any(isinstance(q, (CsrPartition, DeviceCsrPartition)) for q in data.partitions)
        sdt = self._storage_dtype()
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            with self.ctx.engine_lock:
                rows, offs, counts, nnz = self._cell_select(lb, ub, complement, seed, seeding)
                m0 = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
                M = int(m0[-1])
                y = torch.empty(M, dtype=torch.float64, device=self.dev)
                ys = [y[int(m0[i]): int(m0[i + 1])] for i in range(self.n_local)]
                if csr:
                    z0 = np.concatenate([[0], np.cumsum(nnz, dtype=np.int64)]).astype(np.int64)
                    rp = torch.empty(M + max(self.n_local, 1), dtype=torch.int64, device=self.dev)
                    col = torch.empty(int(z0[-1]), dtype=torch.int32, device=self.dev)
                    val = torch.empty(int(z0[-1]), dtype=sdt, device=self.dev)
                    rps = [rp[int(m0[i]) + i: int(m0[i + 1]) + i + 1] for i in range(self.n_local)]
                    cols = [col[int(z0[i]): int(z0[i + 1])] for i in range(self.n_local)]
                    vals = [val[int(z0[i]): int(z0[i + 1])] for i in range(self.n_local)]
                    if self.n_local > 0:
                        ptr = lambda ts: [t.data_ptr() if t.numel() else 0 for t in ts]
                        self.ctx.gather_csr_device(rows.data_ptr(), counts, nnz, ptr(ys), [t.data_ptr() for t in rps],
                                                   ptr(cols), ptr(vals), self.stream.cuda_stream)
                    local = [DeviceCsrPartition(ys[i], rps[i], cols[i], vals[i], d) for i in range(self.n_local)]
                    arena = (y, rp, col, val)
                    zero = torch.zeros(1, dtype=torch.int64, device=self.dev)
                    empty = lambda: DeviceCsrPartition(y[:0], zero, col[:0], val[:0], d)
                else:
                    vec = 4 if sdt == torch.float32 else 2
                    ld = (d + vec - 1) // vec * vec
                    X = torch.empty((M, ld), dtype=sdt, device=self.dev)
                    xs = [X[int(m0[i]): int(m0[i + 1])] for i in range(self.n_local)]
                    if self.n_local > 0:
                        ptr = lambda ts: [t.data_ptr() if t.numel() else 0 for t in ts]
                        self.ctx.gather_dense_device(rows.data_ptr(), counts, ld, ptr(xs), ptr(ys),
                                                     self.stream.cuda_stream)
                    local = [DevicePartition(ys[i], xs[i], d) for i in range(self.n_local)]
                    arena = (y, X)
                    empty = lambda: DevicePartition(y[:0], X[:0], d)
            part_counts = np.zeros(P, dtype=np.int64)
            if self.world > 1:
                import torch.distributed as dist
                shards = [shard_range(P, r, self.world) for r in range(self.world)]
                width = max(max(hi - lo for lo, hi in shards), 1)
                buf = torch.zeros(width, dtype=torch.int64, device=self.dev)
                buf[: self.n_local].copy_(torch.from_numpy(counts))
                got = torch.empty(self.world * width, dtype=torch.int64, device=self.dev)
                if dist.get_backend() == "gloo":
                    dist.all_gather(list(got.view(self.world, width).unbind(0)), buf)
                else:
                    dist.all_gather_into_tensor(got, buf)
                h = got.cpu().numpy().reshape(self.world, width)
                for r, (lo, hi) in enumerate(shards):
                    part_counts[lo:hi] = h[r, : hi - lo]
            else:
                part_counts[self.lo: self.hi] = counts
        caller.wait_stream(self.stream)
        for t in arena:
            t.record_stream(caller)
        parts = [empty() for _ in range(self.lo)] + local + [empty() for _ in range(P - self.hi)]
        out = PartitionedData(parts)
        out.partition_counts = part_counts
        return out

    # the row projection (psgd_project_device; stat.multiply, feature.PCAModel) ---------------------
    def project(self, B, storage=None) -> PartitionedData:
        """Y = X B for B [d, k] (a numpy array or a device tensor), as a PartitionedData of dense device
        partitions of k features built the way split_cell builds its result: one arena, this rank's
        block filled by one launch over all its partitions (partition p holds the rows of source
        partition p in order, with their labels), empty placeholders for the other ranks' partitions,
        and `partition_counts`, every partition's row count on every rank. storage ("f32" / "f64" or a
        torch dtype; None keeps the source's) is the result's dtype: the fp64 product rounded once.
        The rows come from the context's registered copy: a source column_transform is in them, the
        result carries none."""
        torch = self.torch
        data, P, d = self._data, self._data.num_partitions, self._data.num_features
        if torch.is_tensor(B):
            _require(B.dim() == 2 and B.shape[0] == d, f"B must be [{d}, k] (got {tuple(B.shape)})")
        else:
            B = np.asarray(B, dtype=np.float64)
            _require(B.ndim == 2 and B.shape[0] == d, f"B must be [{d}, k] (got {B.shape})")
        k = int(B.shape[1])
        _require(1 <= k <= N.PROJECT_MAX_K, f"a projection takes 1 <= k <= {N.PROJECT_MAX_K} components (got {k})")
        if storage is None:
            odt = self._storage_dtype()
        else:
            odt = {"f32": torch.float32, "f64": torch.float64, torch.float32: torch.float32,
                   torch.float64: torch.float64}.get(storage)
            _require(odt is not None, f"storage must be 'f32', 'f64' or None (got {storage!r})")
        n_rows = np.array([data.partitions[p].n_rows for p in range(self.lo, self.hi)], dtype=np.int64)
        m0 = np.concatenate([[0], np.cumsum(n_rows, dtype=np.int64)]).astype(np.int64)
        M = int(m0[-1])
        vec = 4 if odt == torch.float32 else 2
        ld = (k + vec - 1) // vec * vec
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            if torch.is_tensor(B):
                b_dev = B.to(device=self.dev, dtype=torch.float64).contiguous()
            else:
                b_dev = torch.from_numpy(np.ascontiguousarray(B)).to(self.dev)
            y = torch.empty(M, dtype=torch.float64, device=self.dev)
            Y = torch.empty((M, ld), dtype=odt, device=self.dev)
            ys = [y[int(m0[i]): int(m0[i + 1])] for i in range(self.n_local)]
            xs = [Y[int(m0[i]): int(m0[i + 1])] for i in range(self.n_local)]
            if M > 0:
                with self.ctx.engine_lock:
                    if self.ctx.registered_token != self._key:
                        self._register(self._data)
                    ptr = lambda ts: [t.data_ptr() if t.numel() else 0 for t in ts]
                    self.ctx.project_device(k, b_dev.data_ptr(), N.F32 if odt == torch.float32 else N.F64, ld,
                                            ptr(xs), ptr(ys), self.stream.cuda_stream)
            keep = torch.cuda.Event()
            keep.record(self.stream)
        caller.wait_stream(self.stream)
        for t in (y, Y):
            t.record_stream(caller)
        keep.synchronize()   # b_dev may be a temporary of this call
        local = [DevicePartition(ys[i], xs[i], k) for i in range(self.n_local)]
        empty = lambda: DevicePartition(y[:0], Y[:0], k)
        part_counts = getattr(data, "partition_counts", None)
        if part_counts is None:
            part_counts = np.array([q.n_rows for q in data.partitions], dtype=np.int64)
        out = PartitionedData([empty() for _ in range(self.lo)] + local + [empty() for _ in range(P - self.hi)])
        out.partition_counts = np.array(part_counts, dtype=np.int64)
        return out


def merge_gradient_sums(rows):
    """Rows of {gradientSum[d], lossSum, count}, one a rank, added in row order: ((r0 + r1) + r2) + ..
    (host arrays or device tensors)."""
    total = rows[0] + 0.0
    for r in range(1, len(rows)):
        total = total + rows[r]
    return total


def merge_column_stats(h: np.ndarray, d: int) -> "ColumnStats":
    """Rows of {count, mean[d], m2[d], numNonzeros[d], max[d], min[d]} merged in row order with
    Chan's formula in fp64 (MultivariateOnlineSummarizer.merge); rows with count 0 are skipped."""
    n = 0.0
    mean = m2 = nnz = mx = mn = None
    for row in np.asarray(h, dtype=np.float64).reshape(-1, 1 + 5 * d):
        nb = float(row[0])
        if nb == 0.0:
            continue
        b = row[1:].reshape(5, d)
        if n == 0.0:
            n, mean, m2, nnz, mx, mn = nb, b[0].copy(), b[1].copy(), b[2].copy(), b[3].copy(), b[4].copy()
            continue
        tot = n + nb
        delta = b[0] - mean
        mean = mean + delta * (nb / tot)
        m2 = m2 + b[1] + delta * delta * (n * nb / tot)
        nnz = nnz + b[2]
        mx = np.maximum(mx, b[3])
        mn = np.minimum(mn, b[4])
        n = tot
    if n == 0.0:
        raise IllegalArgumentException("requirement failed: Nothing has been added to this summarizer.")
    variance = m2 / (n - 1.0) if n > 1.0 else np.zeros(d)
    return ColumnStats(int(n), mean, variance, nnz.astype(np.int64), mx, mn)


EngineScore = collections.namedtuple("EngineScore", "lossSum count nCorrect partLoss partCorrect")
# Statistics.colStats (MultivariateStatisticalSummary): count, and per feature mean, the unbiased
# variance, numNonzeros, max and min.
ColumnStats = collections.namedtuple("ColumnStats", "count mean variance numNonzeros max min")


class Evaluation:
    """A model scored on a data set: lossSum and count over every row, meanLoss = lossSum / count,
    regVal = updater.compute(w, 0, 0, 1, regParam)._2 (the reference's own definition,
    ParallelizedSGD.scala:231-233), objective = meanLoss + regVal, accuracy = nCorrect / count at
    MLlib's default thresholds (None for LeastSquaresGradient), and the per-partition partLoss /
    partCorrect. With count == 0, meanLoss and objective are NaN and accuracy is None."""

    def __init__(self, lossSum: float, count: int, nCorrect: Optional[int], regVal: float,
                 partLoss=(), partCorrect=()):
        self.lossSum = float(lossSum)
        self.count = int(count)
        self.nCorrect = None if nCorrect is None else int(nCorrect)
        self.regVal = float(regVal)
        self.partLoss = np.asarray(partLoss, dtype=np.float64)
        self.partCorrect = np.asarray(partCorrect, dtype=np.int64)

    @property
    def meanLoss(self) -> float:
        return self.lossSum / self.count if self.count > 0 else float("nan")

    @property
    def objective(self) -> float:
        return self.meanLoss + self.regVal

    @property
    def accuracy(self) -> Optional[float]:
        if self.nCorrect is None or self.count == 0:
            return None
        return self.nCorrect / self.count

    def __repr__(self) -> str:
        return (f"Evaluation(lossSum={self.lossSum!r}, count={self.count}, meanLoss={self.meanLoss!r}, "
                f"regVal={self.regVal!r}, objective={self.objective!r}, accuracy={self.accuracy!r})")


def evaluate(data: PartitionedData, gradient: Gradient, updater: SGDUpdater, regParam: float, weights,
             *, engine=None) -> Evaluation:
    """Score `weights` (a host array or a device tensor of num_features doubles) on `data`: the
    true loss and objective at those weights -- not the training's running chain loss -- and the
    accuracy of the classifiers (Evaluation).

    The engine reuses the device context's registration when it holds this data already, so
    scoring the training set after training copies nothing. Scoring another PartitionedData (a
    held-out set) registers it in the training set's place, as any second engine on the device
    does; training on the first set afterwards registers that one again. The multinomial
    LogisticGradient (numClasses > 2) raises UnsupportedOperationException: evaluate_multinomial scores it."""
    if num_classes(gradient) > 2:
        raise N.UnsupportedOperationException(
            "evaluate with the multinomial LogisticGradient (numClasses > 2) is not built: "
            "use evaluate_multinomial")
    gradient_kind(gradient)
    classifier = not isinstance(gradient, LeastSquaresGradient)
    if data.num_partitions == 0:
        return Evaluation(0.0, 0, 0 if classifier else None, float("nan"))
    if engine is None:
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world)
    score = engine.evaluate(gradient, weights)
    w_host = engine.to_host(weights) if hasattr(weights, "data_ptr") else np.asarray(weights, dtype=np.float64)
    params = make_params(gradient, updater, 1.0, regParam, 1.0, 0.0)
    regVal = engine.initial_regval(params, np.ascontiguousarray(w_host, dtype=np.float64))
    return Evaluation(score.lossSum, score.count, score.nCorrect if classifier else None, regVal,
                      score.partLoss, score.partCorrect)


def check_num_classes(numClasses) -> int:
    """K of the multinomial scoring calls: an integer > 2."""
    K = int(numClasses)
    if K < 3:
        raise IllegalArgumentException(
            f"requirement failed: the multinomial scoring calls need numClasses > 2 but got {K} "
            "(a binary model goes through evaluate / predict)")
    return K


def check_multinomial_weights(K: int, num_features: int, size: int) -> None:
    """LogisticGradient.compute: require(weights.size % dataSize == 0 &&
    numClasses == weights.size / dataSize + 1) [ext MLlib 1.6.1]."""
    if num_features == 0 or size < 0 or size % num_features != 0 or K != size // num_features + 1:
        raise IllegalArgumentException("requirement failed")


def _weights_size(weights) -> int:
    shape = tuple(weights.shape) if hasattr(weights, "shape") else np.asarray(weights).shape
    return int(shape[0]) if len(shape) == 1 else -1


def evaluate_multinomial(data: PartitionedData, gradient: Gradient, updater: SGDUpdater, regParam: float, weights,
                         *, engine=None) -> Evaluation:
    """evaluate() for LogisticGradient(numClasses = K > 2): score the (K - 1) * num_features
    `weights` (a host array or a device tensor) on `data` -- the loss of LogisticGradient.compute
    summed, the accuracy of LogisticRegressionModel.predict's classes (the pivot class 0 unless a
    margin is positive; exact ties to the lowest class) and regVal as evaluate() defines it. The
    rows are scored where they are registered; a binary gradient raises IllegalArgumentException."""
    if not isinstance(gradient, LogisticGradient) or num_classes(gradient) < 3:
        raise IllegalArgumentException(
            "requirement failed: evaluate_multinomial needs LogisticGradient(numClasses > 2); "
            "a binary gradient goes through evaluate")
    K = num_classes(gradient)
    if data.num_partitions == 0:
        return Evaluation(0.0, 0, 0, float("nan"))
    check_multinomial_weights(K, data.num_features, _weights_size(weights))
    if engine is None:
        rank, world, _ = _dist()
        engine = HipEngine(data, rank, world)
    score = engine.evaluate_multinomial(K, weights)
    w_host = engine.to_host(weights) if hasattr(weights, "data_ptr") else np.asarray(weights, dtype=np.float64)
    params = make_params(gradient, updater, 1.0, regParam, 1.0, 0.0)
    regVal = engine.initial_regval(params, np.ascontiguousarray(w_host, dtype=np.float64))
    return Evaluation(score.lossSum, score.count, score.nCorrect, regVal, score.partLoss, score.partCorrect)


# ---------------------------------------------------------------------------------------------
# The optimizer.
# ---------------------------------------------------------------------------------------------
class ParallelizedSGD:
    """:: Experimental :: Parallelized Stochastic Gradient Descent (Zinkevich et al.).

    Mirrors ParallelizedSGD.scala:41-159: same defaults (:46-50), same validated setters
    (:56-134, same messages), optimize(data, initialWeights) -> weights (:144-157)."""

    def __init__(self, gradient: Gradient, updater: SGDUpdater):
        self.gradient = gradient
        self.updater = updater
        self.stepSize = 1.0
        self.numIterations = 100
        self.regParam = 0.0
        self.miniBatchFraction = 1.0
        self.convergenceTol = 0.001
        self.compute_dtype = "f64"

    def setStepSize(self, step: float) -> "ParallelizedSGD":
        _require(step > 0, f"Initial step size must be positive but got {_jstr(float(step))}")
        self.stepSize = float(step)
        return self

    def setMiniBatchFraction(self, fraction: float) -> "ParallelizedSGD":
        _require(fraction > 0 and fraction <= 1.0,
                 f"Fraction for mini-batch SGD must be in range (0, 1] but got {_jstr(float(fraction))}")
        self.miniBatchFraction = float(fraction)
        return self

    def setNumIterations(self, iters: int) -> "ParallelizedSGD":
        _require(iters >= 0, f"Number of iterations must be nonnegative but got {iters}")
        self.numIterations = int(iters)
        return self

    def setRegParam(self, regParam: float) -> "ParallelizedSGD":
        _require(regParam >= 0,
                 f"Regularization parameter must be nonnegative but got {_jstr(float(regParam))}")
        self.regParam = float(regParam)
        return self

    def setConvergenceTol(self, tolerance: float) -> "ParallelizedSGD":
        _require(tolerance >= 0.0 and tolerance <= 1.0,
                 f"Convergence tolerance must be in range [0, 1] but got {_jstr(float(tolerance))}")
        self.convergenceTol = float(tolerance)
        return self

    def setGradient(self, gradient: Gradient) -> "ParallelizedSGD":
        self.gradient = gradient
        return self

    def setUpdater(self, updater: SGDUpdater) -> "ParallelizedSGD":
        self.updater = updater
        return self

    def setComputeDtype(self, dtype: str) -> "ParallelizedSGD":
        """Build extension: "f64" (reference arithmetic, default) or "f32" (throughput mode)."""
        _require(dtype in ("f64", "f32"), f"compute dtype must be f64 or f32 but got {dtype}")
        self.compute_dtype = dtype
        return self

    def optimize(self, data: PartitionedData, initialWeights) -> np.ndarray:
        weights, _ = ParallelizedSGD.runParallelizedSGD(
            data, self.gradient, self.updater, self.stepSize, self.numIterations, self.regParam,
            self.miniBatchFraction, initialWeights, self.convergenceTol,
            compute_dtype=self.compute_dtype)
        return weights

    def evaluate(self, data: PartitionedData, weights, *, engine=None) -> "Evaluation":
        """Score `weights` on `data` with this optimizer's gradient, updater and regParam: the loss
        and objective at those weights, the accuracy of a classifier, per-partition sums
        (evaluate() below; build extension, the reference's users go through MLlib's models)."""
        return evaluate(data, self.gradient, self.updater, self.regParam, weights, engine=engine)

    def evaluate_multinomial(self, data: PartitionedData, weights, *, engine=None) -> "Evaluation":
        """evaluate() for this optimizer's LogisticGradient(numClasses > 2) (evaluate_multinomial() below)."""
        return evaluate_multinomial(data, self.gradient, self.updater, self.regParam, weights, engine=engine)

    # object ParallelizedSGD ---------------------------------------------------------------------
    @staticmethod
    def runParallelizedSGD(data: PartitionedData, gradient: Gradient, updater: SGDUpdater,
                           stepSize: float, numIterations: int, regParam: float,
                           miniBatchFraction: float, initialWeights, convergenceTol: float = 0.001,
                           *, compute_dtype: str = "f64", engine=None,
                           return_chain_counts: bool = False,
                           checkpoint: Optional[str] = None, checkpoint_every: int = 1):
        """ParallelizedSGD.scala:188-306 (and the 8-argument alias :311-321 via the default).
        Returns (weights, stochasticLossHistory) [, per-iteration chain counts].

        checkpoint: a file path (extension): the loop state is saved there every
        `checkpoint_every` iterations and after the last one, and a run that finds a checkpoint of
        the same parameters and data resumes from it (DriverCheckpoint). The chain counts of
        iterations before the resume are not in it."""
        if miniBatchFraction < 1.0 and convergenceTol > 0.0:  # :200-203
            log.warning("Testing against a convergenceTol when using miniBatchFraction "
                        "< 1.0 can be unstable because of the stochasticity in sampling.")
        history: List[float] = []
        chain_counts: List[np.ndarray] = []
        w0 = np.ascontiguousarray(np.asarray(initialWeights, dtype=np.float64))

        numExamples = data.count()  # :211
        if numExamples == 0:  # :214-217
            log.warning("GradientDescent.runMiniBatchSGD returning initial weights, no data found")
            out = (w0, np.array(history))
            return out + (chain_counts,) if return_chain_counts else out
        if numExamples * miniBatchFraction < 1:  # :219-221
            log.warning("The miniBatchFraction is too small")
        nf = data.num_features
        if isinstance(gradient, LogisticGradient):
            # LogisticGradient.compute: require(weights.size % dataSize == 0 &&
            # numClasses == weights.size / dataSize + 1) [ext MLlib 1.6.1]
            if nf == 0 or w0.shape[0] % nf != 0 or num_classes(gradient) != w0.shape[0] // nf + 1:
                raise IllegalArgumentException("requirement failed")
        elif w0.shape[0] != nf:
            raise IllegalArgumentException(
                f"requirement failed: BLAS.dot(x: Vector, y: Vector) was given Vectors with "
                f"non-matching sizes: x.size = {nf}, y.size = {w0.shape[0]}")

        if engine is None:
            rank, world, _ = _dist()
            engine = HipEngine(data, rank, world, weight_dim=weight_dim(gradient, nf))

        params = make_params(gradient, updater, stepSize, regParam, miniBatchFraction,
                             convergenceTol, compute_dtype)
        ckpt = DriverCheckpoint(checkpoint, checkpoint_every) if checkpoint else None
        fp = _ckpt_fingerprint(params, data, w0) if ckpt else None
        state = ckpt.load(fp) if ckpt else None
        if state is None:
            weights = engine.weights(w0)                  # :224
            regVal = engine.initial_regval(params, w0)    # :231-233
            have_current = False
            converged = False
            i = 1
        else:
            weights = engine.weights(state["weights"])
            regVal, history = state["regVal"], state["history"]
            have_current, converged, i = state["have_current"], state["converged"], state["i"]
            log.warning("resuming at iteration %d from checkpoint %s", i, checkpoint)
        last_saved = i
        if (convergenceTol == 0.0 and miniBatchFraction >= 1.0 and ckpt is None and not return_chain_counts
                and hasattr(engine, "epoch_async")):
            weights, regVal = ParallelizedSGD._run_pipelined(engine, params, weights, regVal, i,
                                                             numIterations, history)
            i = numIterations + 1
        while not converged and i <= numIterations:       # :237
            params.iteration = i
            folded, counts = engine.epoch(params, weights, with_counts=return_chain_counts)
            avgRegVal, lossSum, batchSize = engine.scalars(folded)
            if return_chain_counts:
                chain_counts.append(counts)
            if batchSize > 0:                              # :278
                stochasticLoss = lossSum / batchSize + regVal   # :283
                history.append(stochasticLoss)
                log.warning("stochastic loss at step%d: %s", i, stochasticLoss)
                new_weights = engine.adopt(folded)         # :286-287
                regVal = avgRegVal
                if have_current:                           # :289-294
                    dsq, nsq = engine.convergence_terms(weights, new_weights)
                    converged = math.sqrt(dsq) < convergenceTol * max_j(math.sqrt(nsq), 1.0)
                weights = new_weights
                have_current = True
            else:                                          # :295-297
                log.warning("Iteration (%d/%d). The size of sampled batch is zero", i, numIterations)
            i += 1
            if ckpt and (i - last_saved >= ckpt.every or converged or i > numIterations):
                ckpt.save(fp, engine.to_host(weights), i, regVal, history, have_current, converged)
                last_saved = i
        log.info("GradientDescent.runMiniBatchSGD finished. Last 10 stochastic losses %s",
                 ", ".join(str(v) for v in history[-10:]))
        out = (engine.to_host(weights), np.array(history))
        return out + (chain_counts,) if return_chain_counts else out

    # (the number of epochs enqueued ahead of the one whose scalars are read)
    PIPELINE_LAG = 2

    @staticmethod
    def _run_pipelined(engine, params, weights, regVal: float, i: int, numIterations: int,
                       history: List[float]):
        """The loop :237-297 when its branches are known before an epoch's scalars are: with
        convergenceTol == 0 `isConverged` (:324-336) is `norm < 0.0 * max(.)`, never true, and
        with miniBatchFraction == 1 every row of the (non-empty, :214-217) data is in every batch
        (:242), so batchSize > 0 (:278) and the folded weights are always adopted (:286). Each
        epoch is enqueued with the previous epoch's folded weights before that epoch's three
        scalars are read back, up to PIPELINE_LAG epochs ahead, so the device runs epoch after
        epoch without waiting for the host; the loss history, regVal lag (:283, :287) and log
        lines follow in iteration order as each epoch's scalars arrive. Returns (weights, regVal)."""
        pending = collections.deque()

        def settle(regVal):
            it, token = pending.popleft()
            avgRegVal, lossSum, batchSize = engine.scalars_wait(token)
            if batchSize <= 0:   # a full batch of non-empty data: cannot happen
                raise RuntimeError(f"iteration {it}: an empty batch in a full-batch epoch")
            stochasticLoss = lossSum / batchSize + regVal          # :283
            history.append(stochasticLoss)
            log.warning("stochastic loss at step%d: %s", it, stochasticLoss)
            return avgRegVal                                       # :287

        try:
            while i <= numIterations:
                params.iteration = i
                folded, token = engine.epoch_async(params, weights)
                pending.append((i, token))
                # (valid while the next epoch reads it; every later use is after its own epoch)
                weights = engine.adopt_view(folded)                # :286
                if len(pending) > ParallelizedSGD.PIPELINE_LAG:
                    regVal = settle(regVal)
                i += 1
            while pending:
                regVal = settle(regVal)
        except BaseException:
            # epochs still in flight write their scalars to the engine's page-locked slots:
            # let them finish before the error unwinds (and may free the engine)
            if hasattr(engine, "drain"):
                engine.drain()
            raise
        # the last epoch's weights, copied out of the alternating result buffers
        return engine.adopt(weights), regVal


_CKPT_VERSION = 1


def _ckpt_fingerprint(params, data: PartitionedData, w0: np.ndarray) -> np.ndarray:
    """What an iteration's result depends on besides (w, i): the plugins and hyper-parameters
    (the psgd_params fields), the data's shape and column transform, the initial weights (the first regVal and the
    driver's first convergence reference). numIterations is left out, so a finished run can be
    resumed with a larger iteration budget and continue exactly where it stopped."""
    import hashlib
    h = hashlib.sha256()
    for f, _ in N.psgd_params._fields_:
        if f != "iteration":
            h.update(f"{f}={getattr(params, f)!r};".encode())
    h.update(f"n={data.count()};P={data.num_partitions};d={data.num_features};".encode())
    h.update(np.ascontiguousarray(w0, dtype=np.float64).tobytes())
    # a column transform the data carries (StandardScalerModel.transform) changes every row the
    # chains read: a checkpoint of scaled data must not resume on unscaled data
    tr = getattr(data, "column_transform", None)
    if tr is not None:
        shift, factor = tr
        h.update(b"transform;shift=" + (b"none" if shift is None else
                                       np.ascontiguousarray(shift, dtype=np.float64).tobytes()))
        h.update(b";factor=" + np.ascontiguousarray(factor, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


class DriverCheckpoint:
    """Checkpoint / resume of the driver loop (the reference has none and returns the
    weights only, ParallelizedSGD.scala:304). The loop's whole state between iterations is
    (weights, i, regVal, stochasticLossHistory, whether `currentWeights` is defined, converged):
    an epoch is a pure function of (weights, i, data) -- the sample seed is 42 + i (:240), every
    chain starts its updater status afresh (:246) -- so a resumed run continues bit for bit.

    Written by rank 0 only (every rank holds the same folded state), atomically (temp file +
    os.replace), as an .npz read back with allow_pickle=False."""

    def __init__(self, path: str, every: int = 1):
        _require(every >= 1, f"checkpoint interval must be positive but got {every}")
        self.path, self.every = str(path), int(every)

    def load(self, fingerprint: np.ndarray):
        """The saved loop state, or None. With world > 1 only rank 0 reads the file (it is the
        rank that writes it; other ranks may see a node-local path or none) and broadcasts the
        state, so every rank resumes at the same iteration; a rank whose own parameter/data
        fingerprint differs from rank 0's makes every rank raise, rather than issue mismatched
        collectives. The fingerprint covers the parameters, the data's shape and the initial
        weights, not the data's values."""
        rank, world, _ = _dist()
        state, err = None, None
        if rank == 0:
            try:
                state = self._read(fingerprint)
            except IllegalArgumentException as e:
                err = str(e)
            except Exception as e:   # unreadable file (truncated zip, old format, I/O error):
                # forwarded, so every rank raises after the broadcast instead of ranks >= 1
                # waiting in it for the process-group timeout
                err = f"checkpoint {self.path}: unreadable ({e!r})"
        if world > 1:
            import torch.distributed as dist
            box = [(state, err, np.asarray(fingerprint).tobytes())]
            dist.broadcast_object_list(box, src=0)
            state, err, fp0 = box[0]
            agree = [None] * world
            dist.all_gather_object(agree, fp0 == np.asarray(fingerprint).tobytes())
            if err is None and not all(agree):
                err = (f"checkpoint {self.path}: ranks {[r for r, a in enumerate(agree) if not a]} "
                       f"run with other parameters or data than rank 0")
        if err is not None:
            raise IllegalArgumentException(err)
        return state

    def _read(self, fingerprint: np.ndarray):
        import os
        if not os.path.exists(self.path):
            return None
        with np.load(self.path, allow_pickle=False) as z:
            if int(z["version"]) != _CKPT_VERSION or not np.array_equal(z["fingerprint"], fingerprint):
                raise IllegalArgumentException(
                    f"checkpoint {self.path} was written by a run with other parameters or data")
            return dict(weights=z["weights"].copy(), i=int(z["i"]), regVal=float(z["regVal"]),
                        history=[float(v) for v in z["history"]],
                        have_current=bool(z["have_current"]), converged=bool(z["converged"]))

    def save(self, fingerprint, weights_host, i, regVal, history, have_current, converged):
        import os
        rank, _, _ = _dist()
        if rank != 0:
            return
        tmp = f"{self.path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            np.savez(f, version=np.int64(_CKPT_VERSION), fingerprint=fingerprint,
                     weights=np.asarray(weights_host, dtype=np.float64), i=np.int64(i),
                     regVal=np.float64(regVal), history=np.asarray(history, dtype=np.float64),
                     have_current=np.bool_(have_current), converged=np.bool_(converged))
        os.replace(tmp, self.path)


def max_j(a: float, b: float) -> float:
    """java.lang.Math.max (NaN-propagating)."""
    if a != a:
        return a
    if b != b:
        return b
    return a if a >= b else b


runParallelizedSGD = ParallelizedSGD.runParallelizedSGD
