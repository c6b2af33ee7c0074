"""Planner and executor for the HIP path: a recorded layer graph becomes one launch list, run by one FFI call.

A model describes its forward once, symbolically, through ``Recorder`` (the model's ``_trace`` method reads like the
reference's ``_forward_encoder``).  ``Plan`` then runs these passes, in this order:

1. graph.py - ``Recorder`` / ``Sym`` / ``Node``: the recorded layers.  ``Node.attrs`` is the recorder's; no pass writes to it.
2. planner.fuse - the fusion rules, one matcher each, listed once in ``planner.RULES`` (the order is the priority): which
   nodes become which launch.  The result is one typed ``Launch`` record per launch.  A new fusion is a matcher there, a
   line in that table and (for a new kernel) an emitter in emit.py.
3. planner.place / planner.alloc - where every activation lives, so that the reference's element-wise glue disappears into
   the convolution epilogues:
   * ``Concat`` (reference models/yolo_layer.py:16-22): every input is produced straight into its channel slice of one NHWC
     buffer;
   * ``Upsample(2)`` (:6-13): folded into the producing conv's store (2x2 replicate);
   * ``Add`` (models/yolov3_spp.py:12-14): residual read in the conv epilogue, written in place of the residual input; the
     pre-add branch output the reference routes to the FPN (yolov3_spp.py:42-46) is a second epilogue store;
   * SPP ``cat([p5,p9,p13,x])`` (yolov3_spp.py:129): conv writes x into the last slice, one kernel fills the other three;
   then storage, shared between buffers whose live ranges do not overlap.
4. emit.build_ops - one emitter per launch kind turns the records into the ``YoloOp`` array (both precisions).
5. diag.py - the opt-in diagnostics: list rewrites after emission (YOLO_SHRINK_OPS, YOLO_DEPTH_FIRST) and the red-zone
   allocator (YOLO_REDZONE).

This file is the executor: ``Plan`` (one ``yolo_run_ops`` FFI call for all layers + one decode launch per head that does not
decode in its conv, optionally captured in a HIP graph), ``StreamedPlan`` (sub-batches / whole batches on several streams) and
``FastStep`` (the one-call pipeline step of ``detect_stream()``).
"""
from __future__ import annotations

import atexit
import ctypes as C
import os

import torch

from . import emit, planner
from . import kernels as K
from ._lib import YoloOp
from .diag import DEPTH_FIRST_DEFAULT, GuardedAlloc                     # noqa: F401 (public names of this module)
from .graph import Buf, Node, Recorder, Sym                             # noqa: F401
from .planner import FUSE_RESUNIT_DEFAULT, Launch                       # noqa: F401


class _Runs:
    """What Plan and StreamedPlan share: output buffers for a batch of ``bs`` images, the eager run and the HIP-graph replay
    (both through the class's own ``_launch``)."""
    def new_outputs(self, want_p: bool = True):
        """io and the raw head tensors p.  ``want_p=False`` (detect(): NMS reads io only) leaves p out: the head kernels then
        skip its store (0.87 GB per 32 SPP-640 images) - p is ``(None, ...)``."""
        no = self.n_class + 5
        io = torch.empty((self.bs, self.rows_total, no), dtype=torch.float32, device=self.device)
        ps = tuple(torch.empty((self.bs, hd["na"], hd["sym"].h, hd["sym"].w, no), dtype=torch.float32, device=self.device) if want_p else None
                   for hd in self.heads)
        return io, ps

    def run(self, x: torch.Tensor):
        """Eager launch on the current stream; returns fresh (io, p) tensors."""
        io, ps = self.new_outputs()
        self._launch(x, io, ps)
        return io, ps

    def run_graph(self, x: torch.Tensor):
        """Replay the whole forward (pack + layers + decodes) as one captured HIP graph.
        Returns STATIC output tensors: they are overwritten by the next call."""
        if self._graph is None:
            self._static_x = torch.empty_like(x)
            self._static_out = self.new_outputs()
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                    # warm-up outside capture
                self._static_x.copy_(x)
                self._launch(self._static_x, *self._static_out)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._launch(self._static_x, *self._static_out)
            self._graph = graph
        self._static_x.copy_(x)
        self._graph.replay()
        return self._static_out


# ------------------------------------------------------------------------------------------------
class Plan(GuardedAlloc, _Runs):
    """Buffers + packed weights + launch list for one (batch, H, W) on one device.

    ``precision``: "bf16" (default: bf16 activations / weights, fp32 accumulate, every fusion), "fp32" (the
    reference-precision parity mode: float32 activations and weights on the f32 MFMA, one plain launch per layer,
    csrc/conv_f32.hip) or "fp16" (the rounding points of the bf16 mode with IEEE-half activations / weights: three more
    mantissa bits at the bf16 MFMA rate; one launch per layer - the 20x20-tile kernels on the large 3x3 layers, the gather kernel elsewhere -, heads decoded in their conv, the Darknet
    families only)."""
    n_streams = 1

    def __init__(self, rec: Recorder, device, n_class: int, img_size: int, precision: str = "bf16"):
        if precision not in ("bf16", "fp32", "fp16"):
            raise ValueError(f"precision must be 'bf16', 'fp32' or 'fp16', got {precision!r}")
        self.f32 = precision == "fp32"
        self.f16 = precision == "fp16"
        self.precision = precision
        self.device = device
        self.rec = rec
        self.bs = rec.input.n
        self.n_class = n_class
        self.img_size = img_size
        self._keep = []                 # packed weights / biases kept alive
        self._redzones = []             # (YOLO_REDZONE: GuardedAlloc)
        self._compact_ws = None         # compact NMS workspace, made on first use
        self._bound = None              # what the head ops currently point at (_bind_outputs)
        self._graph = None
        self._static_out = None
        self.depth_first, self._x_patch = [], [(0, 0)]
        self.launches = planner.fuse(rec, self.f32, n_class, self.f16)
        self.fused_input = any(L.reads_nchw for L in self.launches)
        self._bufs = planner.place(rec, self.launches)
        self.shared_buffers = planner.alloc(rec, self.launches, self._bufs, self.f32, self._zeros, self.f16)
        emit.build_ops(self)            # -> heads, rows_total, op_array, n_ops, op_launches, op_nodes

    def set_input_ptr(self, ptr: int):
        """The first layer reads the caller's float32 NCHW batch itself: point its launch(es) at this call's batch."""
        for idx, off in self._x_patch:
            self.op_array[idx].x = ptr + off

    # -- execution -----------------------------------------------------------------------------------
    @property
    def input_buffer(self) -> torch.Tensor:
        return self.rec.input.buf.tensor

    def feed(self, x: torch.Tensor):
        """Hand the float32 NCHW batch to the layer list: either the first conv reads it directly
        (pointer patched into its op) or it is packed to NHWC (bf16, fp16 or float32: the plan's precision) first."""
        if self.fused_input:
            if x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape[1:]) != (self.rec.c_in, self.rec.input.h, self.rec.input.w):
                raise RuntimeError("input must be contiguous float32 NCHW of the planned shape")
            self.set_input_ptr(x.data_ptr())
        elif self.f32:
            K.pack_input_f32(x, self.input_buffer)
        elif self.f16:
            K.pack_input_f16(x, self.input_buffer)
        else:
            K.pack_input(x, self.input_buffer)

    def _launch(self, x: torch.Tensor, io: torch.Tensor, ps, timing=None, before_io=None, compact=None):
        """pack -> layer list -> decodes on the current stream.  ``timing`` = (start, end) torch events
        recorded around the layer list (bench.py's roofline measurement).  ``before_io()`` is called right before the first
        launch that writes ``io`` (a pipelined caller makes the stream wait there for the previous batch's NMS, which reads it).
        ``compact`` = (workspace, conf_thres, min_wh): the heads filter their rows into the compact NMS workspace instead of
        storing ``io`` (which may be None then); ``before_io`` then guards the workspace the same way."""
        self.feed(x)
        self._bind_outputs(io, ps, compact)
        if timing is not None:
            timing[0].record()
        fused = [hd["op"] for hd in self.heads if hd["op"] is not None]
        k = min(fused) if fused else self.n_ops
        if before_io is None or k == 0:
            if before_io is not None:
                before_io()
            K.run_ops(self.op_array, self.n_ops)
        else:
            K.run_ops(self.op_array, k)
            before_io()
            if k < self.n_ops:
                K.run_ops(C.cast(C.byref(self.op_array, k * C.sizeof(YoloOp)), C.POINTER(YoloOp)), self.n_ops - k)
        if timing is not None:
            timing[1].record()
        self._decode_unfused(io, ps)

    @property
    def compact_ok(self) -> bool:
        """Every head decodes in its conv epilogue (bf16 and fp16 modes): detect() can take the compact NMS form (no io)."""
        return not self.f32 and all(hd["op"] is not None for hd in self.heads)

    def compact_workspace(self) -> torch.Tensor:
        """This plan's compact NMS workspace (survivor counts, keys, staging, records: yolo_nms_compact_workspace_bytes), made once."""
        ws = self._compact_ws
        if ws is None:
            ws = self._compact_ws = torch.empty(K.nms_compact_workspace_bytes(self.rec.input.n, self.rows_total, self.n_class),
                                                dtype=torch.uint8, device=self.device)
        return ws

    def _bind_outputs(self, io, ps, compact=None):
        """Heads that decode in their conv epilogue write io / p themselves: patch this call's buffers into their ops.
        ``compact`` = (workspace, conf_thres, min_wh): they filter into the compact NMS workspace instead and store no io."""
        if compact is not None:
            if not self.compact_ok:
                raise RuntimeError("the compact NMS form needs every head to decode in its conv epilogue")
            ws, conf, min_wh = compact
            for hd, p in zip(self.heads, ps):
                op = self.op_array[hd["op"]]
                op.y, op.y_aux = None, (p.data_ptr() if p is not None else None)
                op.workspace, op.ws_bytes = ws.data_ptr(), ws.numel()
                op.head_filter_conf, op.head_filter_min_wh = float(conf), float(min_wh)
            self._bound = (ws.data_ptr(), float(conf), tuple(None if p is None else p.data_ptr() for p in ps))
            return
        if io.shape[1] != self.rows_total or not io.is_contiguous():
            raise RuntimeError("io must be a contiguous [bs, rows_total, 5+nc] tensor")
        for hd, p in zip(self.heads, ps):
            if hd["op"] is not None:
                op = self.op_array[hd["op"]]
                op.y, op.y_aux = io.data_ptr(), (p.data_ptr() if p is not None else None)
                op.workspace, op.ws_bytes = None, 0
        self._bound = (io.data_ptr(), None, tuple(None if p is None else p.data_ptr() for p in ps))

    def _decode_unfused(self, io, ps):
        for hd, p in zip(self.heads, ps):
            if hd["op"] is None:
                K.decode(hd["sym"].buf.tensor, hd["anchors"], self.n_class, hd["stride"], io, hd["row"], p)

    def launch_detect(self, x, io, ps, nms_out, conf_thres, nms_thres, timing=None, join=True, after_nms=None, whole_batch=False,
                      wait_for=None, compact=False, cu_partition=False, nms_style="MERGE"):
        """forward + decode + NMS (``nms_style``: utils.non_max_suppression) into caller-provided buffers; no host sync (``cu_partition`` / ``whole_batch`` / ``join`` are
        the StreamedPlan's: one list on the current stream has nothing to partition).  ``compact=True``: the compact NMS form
        (``io`` is not written and may be None; include/yolo_hip.h yolo_head_decode_filter_fwd) where the plan allows it.
        nms_out = (dets [bs,cap,7] f32, idx [bs,cap] i32, count [bs] i32).  ``timing``: one (start, end)
        event pair per stream, recorded around the conv launch list.  ``after_nms(i, lo, hi)`` is called in
        the context of stream i right after the NMS launch of images [lo, hi) (see distributed.PipelinedGather)."""
        from ._lib import nms_style_id
        from .utils.utils import MAX_PER_CLASS, MIN_WH, nms_launch
        style = nms_style_id(nms_style)
        if compact and self.compact_ok:
            ws = self.compact_workspace()
            self._launch(x, None, ps, timing=timing[0] if timing else None, compact=(ws, conf_thres, MIN_WH))
            K.nms_styled_compact(ws, x.shape[0], self.rows_total, self.n_class, nms_thres, *nms_out, style=style,
                                 max_per_class=MAX_PER_CLASS)
        else:
            self._launch(x, io, ps, timing=timing[0] if timing else None)
            nms_launch(io, conf_thres, nms_thres, nms_out, slot=0, nms_style=nms_style)
        if after_nms is not None:
            after_nms(0, 0, x.shape[0])


    def conv_flops(self) -> float:
        return emit.conv_flops(self.op_array, self.n_ops, self.rec.c_in)

    def algorithmic_bytes(self, detect: bool = False) -> float:
        return emit.algorithmic_bytes(self.op_array, self.n_ops, self.rec.c_in, detect)

    def activation_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in {b.tensor.data_ptr(): b.tensor for b in self._bufs}.values())


_masked_streams = {}
_streamed_plans = None      # weakref.WeakSet of the StreamedPlans alive (they may hold references to the masked streams)


def destroy_masked_streams():
    """Drain and destroy every CU-masked HIP stream this process created (hipExtStreamCreateWithCUMask has no owner in torch:
    an ExternalStream never destroys its handle).  Registered with ``atexit``: streams still alive when the HIP runtime and a
    profiler's tool library unwind their own state crashed ``rocprofv3`` runs of the partitioned bench inside ``__cxa_finalize``
    (VERDICT r3 item 6).  May also be called between batches (nothing in flight on the partitioned streams - they are drained
    here): every live ``StreamedPlan`` forgets its references to the destroyed handles, so its next partitioned call creates
    new streams instead of enqueueing on destroyed ones."""
    streams = [st for group in _masked_streams.values() for st in group]
    _masked_streams.clear()
    for sp in list(_streamed_plans or ()):
        for attr in ("_pipe_streams", "_full_streams"):
            held = getattr(sp, attr, None)
            if held is not None and any(h is st for h in held for st in streams):
                setattr(sp, attr, None)
                if attr == "_full_streams":
                    sp._full_mode = None
    for st in streams:
        try:
            st.synchronize()
            K.check(K.load().yolo_stream_destroy(C.c_void_p(st.cuda_stream)), "stream_destroy")
        except Exception:                                  # noqa: BLE001 (interpreter teardown: nothing left to report to)
            pass


atexit.register(destroy_masked_streams)


class _launch_cus:
    """with _launch_cus(n): the launches of this thread size their grids for n compute units (None: leave as is)."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = K.set_launch_cus(self.n) if self.n else None

    def __exit__(self, *exc):
        if self.old is not None:
            K.set_launch_cus(self.old)
        return False


def _cu_masked(streams) -> bool:
    """The streams are the CU-masked ones of ``_make_streams`` (torch sees those as ExternalStream), not torch's own."""
    return type(streams[0]).__name__ == "ExternalStream"


class StreamedPlan(_Runs):
    """The batch split into S contiguous sub-batches, each with its own Plan, run on S HIP streams.

    Images are independent, so results are identical; what changes is occupancy: the heavy layers launch
    200..800 tiles of 256x256 on 256 CUs, i.e. 1.56 or 3.1 "rounds", and the partial last round leaves a
    quarter of the chip idle.  Two kernels from two streams fill each other's tails (measured: -9.5 % on
    the SPP-640 bs=32 layer list; four streams are no better than two).  Each stream owns half of every XCD's
    compute units (_make_streams)."""

    def __init__(self, make_plan, bs: int, n_streams: int, device):
        assert bs % n_streams == 0
        self.sub = bs // n_streams
        self.subs = [make_plan(self.sub) for _ in range(n_streams)]
        # joined calls (forward(), detect()): ordinary streams - both sub-batches start together and stay in step, layer for layer,
        # so a CU partition has nothing complementary to overlap and only costs (-6 % on detect()).  Free-running pipelines
        # (launch_detect(join=False): bench.py, a serving loop) drift apart: there each stream owns half of every XCD.
        # The partitioned streams are created on the first pipelined call only: they are BLOCKING streams
        # (hipExtStreamCreateWithCUMask takes no flags), and while any exists every operation on the NULL stream - torch's default
        # current stream - pays for the implicit synchronisation with them (host-bound detect() loop: -5..9 %).
        self.streams = [torch.cuda.Stream(device=device) for _ in range(n_streams)]
        self._pipe_streams = None
        # pipelined calls: the NMS of a sub-batch runs on a stream of its own (all CUs), so the pipeline's stream goes straight on
        # to the next batch's layer list; it waits for that NMS only in front of its first head launch (the next writer of io)
        self._make_plan, self._full, self._full_streams, self._batches = make_plan, None, None, 0
        self._full_mode = None          # cu_partition flag of the last whole-batch call (launch_detect)
        self._fast_events = None
        self._detect_fast = None        # detect_step()'s FastStep (False: this plan cannot take one)
        self._nms_stream = None
        self._nms_streams = None
        self._heads_done = [torch.cuda.Event() for _ in range(n_streams)]
        self._nms_done = [None] * n_streams
        self._marks = [torch.cuda.Event() for _ in range(n_streams)]
        p0 = self.subs[0]
        self.device, self.n_class, self.img_size = device, p0.n_class, p0.img_size
        self.heads, self.rows_total = p0.heads, p0.rows_total
        self.bs = bs
        self._graph = None
        global _streamed_plans
        if _streamed_plans is None:
            import weakref
            _streamed_plans = weakref.WeakSet()
        _streamed_plans.add(self)

    @staticmethod
    def _make_streams(n_streams, device, flops_per_launch=0.0):
        """Each sub-batch stream owns its own compute units: stream i gets CUs [i, i+1) * per_xcd / S of every XCD (CU-mask bit b
        lies on XCD b % 8), so two layer lists really run side by side - one stream's HBM-bound phases (1x1 layers, epilogues)
        under the other's MFMA-dense ones - instead of time-slicing the workgroup slots of the whole chip (a 3x3 launch takes
        every register of every CU it lands on).  It pays where the launches are MFMA-dense and about one round of workgroups
        long - the chip then runs against its socket power limit and half the CUs hold a higher clock.
        Measured images/s, split vs shared: SPP-640 bs=32 +2.6 %, bs=16 +1.5 %, bs=64 -0.7 %; SPP-416 bs=32 -9 %; tiny-416 -2.5 %,
        MobileNetV2-tiny -4.6 % (small launches).  "auto" therefore splits between 16 and 96 GFLOP per launch of a pipeline
        (SPP-640 at 8..32 images per stream); whole XCDs per stream ("xcd") lose 1 %.
        YOLO_CU_PARTITION = auto (default) | split | xcd | off."""
        mode = os.environ.get("YOLO_CU_PARTITION", "auto")
        if mode == "auto":      # (round 3: the whole-batch pipelines of SPP-640 x 32 - 69 GFLOP per launch - gain 1.0 % too: profiles/r03_cu_partition_ab.txt)
            mode = "split" if 16e9 <= flops_per_launch < 96e9 else "off"
        n_cu = torch.cuda.get_device_properties(device).multi_processor_count
        n_xcd = 8
        per = n_cu // n_xcd
        if mode in ("off", "0", "") or n_streams < 2 or n_cu % n_xcd or per % n_streams:
            return [torch.cuda.Stream(device=device) for _ in range(n_streams)]
        if mode == "split":
            sets = [[b for b in range(n_cu) if (b // n_xcd) * n_streams // per == i] for i in range(n_streams)]
        elif mode == "xcd" and n_xcd % n_streams == 0:
            sets = [[b for b in range(n_cu) if (b % n_xcd) * n_streams // n_xcd == i] for i in range(n_streams)]
        else:
            raise RuntimeError(f"YOLO_CU_PARTITION={mode!r}: expected off, split or xcd")
        idx = torch.device(device).index
        key = (torch.cuda.current_device() if idx is None else idx, n_streams, mode)
        if key not in _masked_streams:                      # HIP streams with a CU mask are created once per device and shared by the plans
            _masked_streams[key] = [K.cu_masked_stream(s, device) for s in sets]
        return _masked_streams[key]

    def _launch(self, x, io, ps, timing=None):
        cur = torch.cuda.current_stream()
        if timing is not None:
            timing[0].record(cur)
        self._fork(cur)
        for i, (pl, st) in enumerate(zip(self.subs, self.streams)):
            lo, hi = i * self.sub, (i + 1) * self.sub
            with torch.cuda.stream(st):
                sub_ps = tuple(None if p is None else p[lo:hi] for p in ps)
                pl.feed(x[lo:hi])
                pl._bind_outputs(io[lo:hi], sub_ps)
                K.run_ops(pl.op_array, pl.n_ops)
                self._marks[i].record(st)
                pl._decode_unfused(io[lo:hi], sub_ps)
        if timing is not None:
            for m in self._marks:
                cur.wait_event(m)
            timing[1].record(cur)          # every stream's layer list is done (decodes may still run)
        for st in self.streams:
            cur.wait_stream(st)

    @property
    def pipe_streams(self):
        if self._pipe_streams is None:
            self._pipe_streams = self._masked_or_own(self.subs[0])
        return self._pipe_streams

    def _masked_or_own(self, plan):
        """The CU-masked streams for pipelines that launch ``plan``'s list where ``_make_streams`` partitions, else the SAME
        streams as the joined calls (more streams than hardware queues - 4 by default - end up sharing a queue, and two
        pipelines on one queue run one after the other)."""
        made = self._make_streams(len(self.streams), self.device, plan.conv_flops() / max(1, plan.n_ops))
        return made if _cu_masked(made) else self.streams

    def _whole_batch_plans(self):
        """One whole-batch plan per pipeline, built on first use."""
        if self._full is None:
            with torch.cuda.device(self.device):
                self._full = [self._make_plan(self.bs) for _ in self.streams]
        return self._full

    def _fork(self, cur):
        """Every sub-batch stream waits for the calling stream - ONE event, recorded before anything is launched.  The CU-masked
        streams are blocking streams (hipExtStreamCreateWithCUMask takes no flags): an event recorded on the NULL stream between
        the launches of two of them would wait for the first one's whole pass, and the sub-batches would run one after the other."""
        ev = torch.cuda.Event()
        ev.record(cur)
        for st in self.streams:
            st.wait_event(ev)

    @property
    def n_streams(self):
        return len(self.streams)

    def launch_detect(self, x, io, ps, nms_out, conf_thres, nms_thres, timing=None, join=True, after_nms=None, whole_batch=False,
                      wait_for=None, cu_partition=False, compact=False, nms_style="MERGE"):
        """``nms_style``: the suppression style of either NMS form (utils.non_max_suppression).

        ``compact=True``: the compact NMS form - the heads filter their own rows, ``io`` is neither written nor read and may be
        None (include/yolo_hip.h yolo_head_decode_filter_fwd; +1.7 % on SPP-640 x 32 from the io store alone) - where the plans allow it.

        ``wait_for``: an event every pipeline of this call waits for before its first launch (pipelined calls do not wait for
        the calling stream: pass the event that says ``x`` is ready when another stream produced it).

        ``cu_partition=True`` (whole-batch pipelines only): each pipeline launches on a stream that owns half of every XCD's CUs
        when ``_make_streams`` finds the launches in the range where that pays (+0.4..1 % on SPP-640 x 32).  Opt-in, for loops that
        only queue launches (bench.py): HIP creates CU-masked streams as BLOCKING streams, so every operation on the default stream
        between two calls - the event that says ``x`` is ready, an H2D copy of the next batch - is a barrier between the
        pipelines, and each of them then has half the chip: ``detect_stream()`` fell from 6,190 to 3,850 images/s with it.

        ``whole_batch=True`` (pipelined calls only): this call's WHOLE batch goes down ONE pipeline and successive calls
        alternate between the pipelines - two batches in flight instead of two halves of one.  The launches are twice as large
        (SPP-640: 32 images instead of 16: +3.4 % images/s), a batch takes twice as long to come out, and the caller must hand
        consecutive calls DIFFERENT io / nms_out buffers (a buffer set may be reused every ``n_streams`` calls: the head launches
        of the later batch wait for the NMS of the earlier one).  ``timing`` then records its first event pair only;
        ``after_nms(k, 0, bs)`` gets the pipeline index.

        Otherwise:
        Each stream runs the WHOLE pipeline (pack/conv1 -> layers -> decode -> NMS) of its sub-batch into
        slices of the shared buffers.  With ``join=False`` the calling stream neither waits for the previous
        work nor for this one: successive calls then form S free-running pipelines (in-order per stream, so
        buffer reuse is safe) — the caller synchronises before reading results, and before a joined call on the same plan
        (the pipelines run on their own, CU-partitioned streams: ``pipe_streams``)."""
        from ._lib import nms_style_id
        from .utils.utils import MAX_PER_CLASS, MIN_WH, nms_launch
        style = nms_style_id(nms_style)
        cur = torch.cuda.current_stream()
        whole = whole_batch and not join
        if whole:
            full = self._full or self._whole_batch_plans()
            if cu_partition and self._full_streams is None:
                self._full_streams = self._masked_or_own(full[0])
            streams = self._full_streams if cu_partition else self.streams
            # the whole-batch plans (activations, events, batch counter) are shared by the two stream sets, which are not ordered
            # with each other: a call that flips ``cu_partition`` drains the device first (a rare transition - bench.py
            # makes it once, between its detect_stream() timing and its step loop)
            if self._full_mode is not None and self._full_mode != bool(cu_partition):
                torch.cuda.synchronize(self.device)
            self._full_mode = bool(cu_partition)
            k = self._batches % len(streams)
            self._batches += 1
            work = [(k, full[k], streams[k], 0, self.bs)]
        else:
            streams = self.streams if join else self.pipe_streams
            work = [(i, pl, st, i * self.sub, (i + 1) * self.sub) for i, (pl, st) in enumerate(zip(self.subs, streams))]
        side_nms = not join and os.environ.get("YOLO_NMS_STREAM", "1") != "0"
        if side_nms:
            self._make_nms_streams()
        if join:
            self._fork(cur)
        # a partitioned pipeline (_masked_or_own handed out other streams than our own) launches on its share of the CUs: the tile
        # rules size their grids against it
        share = None
        if not join and streams is not self.streams and os.environ.get("YOLO_RULES_FOR_SHARE", "1") != "0":
            share = torch.cuda.get_device_properties(self.device).multi_processor_count // len(streams)
        for i, pl, st, lo, hi in work:
            sub_ps = tuple(None if p is None else p[lo:hi] for p in ps)
            tm = (timing[0 if whole else i] if timing else None)
            if wait_for is not None:
                st.wait_event(wait_for)
            cmp_ = (pl.compact_workspace(), conf_thres, MIN_WH) if (compact and pl.compact_ok) else None
            sub_io = None if cmp_ is not None else io[lo:hi]
            with torch.cuda.stream(st), _launch_cus(share):
                if not side_nms:
                    pl._launch(x[lo:hi], sub_io, sub_ps, timing=tm, compact=cmp_)
                else:
                    prev = self._nms_done[i]
                    pl._launch(x[lo:hi], sub_io, sub_ps, timing=tm, compact=cmp_,
                               before_io=(lambda prev=prev, st=st: st.wait_event(prev)) if prev is not None else None)
                    self._heads_done[i].record(st)
            nst = self._nms_streams[i % len(self._nms_streams)] if side_nms else st
            with torch.cuda.stream(nst):
                if side_nms:
                    nst.wait_event(self._heads_done[i])
                if cmp_ is not None:
                    K.nms_styled_compact(cmp_[0], hi - lo, pl.rows_total, pl.n_class, nms_thres, *(t[lo:hi] for t in nms_out),
                                         style=style, max_per_class=MAX_PER_CLASS)
                else:
                    nms_launch(io[lo:hi], conf_thres, nms_thres, tuple(t[lo:hi] for t in nms_out), slot=i, nms_style=nms_style)
                if after_nms is not None:
                    after_nms(i, lo, hi)
                if side_nms:
                    if self._nms_done[i] is None:
                        self._nms_done[i] = torch.cuda.Event()
                    self._nms_done[i].record(nst)
        if join:
            for st in self.streams:
                cur.wait_stream(st)

    def _make_nms_streams(self):
        """The NMS side stream, created at HIGH priority and shared by the pipelines: the NMS of a batch (one 1024-thread workgroup
        per image, latency-bound) is the tail of that batch; at equal priority it waited for CUs behind the other pipeline's queued
        conv workgroups.  ONE stream, not one per pipeline (YOLO_NMS_STREAMS=per-pipeline: no faster on any workload, 88.3 k vs
        87.1 k images/s on YOLOv3-tiny): every HIP stream that has been used owns a hardware queue, and with the default stream,
        the two pipeline streams, two NMS streams and - created last - the two CU-masked streams of ``launch_detect(cu_partition=True)``
        the process held more queues than the scheduler runs side by side: the partitioned loop dropped from 6,600 to 5,720 images/s
        whenever ``detect_stream()`` had run before it (tools/dbg/stream_then_loop.py; GPU_MAX_HW_QUEUES = 12 / 16 changed nothing,
        one queue fewer restored it)."""
        if self._nms_streams is None:
            prio = int(os.environ.get("YOLO_NMS_PRIORITY", "-1"))
            if os.environ.get("YOLO_NMS_STREAMS", "1") == "1":
                one = torch.cuda.Stream(device=self.device, priority=prio)
                self._nms_streams = [one for _ in self.streams]
            else:
                self._nms_streams = [torch.cuda.Stream(device=self.device, priority=prio) for _ in self.streams]
            self._nms_stream = self._nms_streams[0]

    # -- the one-call pipeline step (yolo_pipeline_step): what detect_stream() launches per batch ------------------------------
    def fast_pipeline(self, slot: int, io, out, conf_thres, nms_thres):
        """A ``FastStep`` for ring slot ``slot`` (``out`` = (dets, idx, count); ``io`` = None: the compact NMS form, no io at all;
        a tensor: the heads store io there and the plain NMS reads it): the whole-batch launch list of pipeline ``slot % S`` + NMS
        as ONE FFI call per batch, or None when this plan cannot take it (a head that decodes in a launch of its own, an input the
        first layer does not read itself: then ``launch_detect`` does the same work)."""
        k = slot % len(self.streams)
        if not self.subs[0].fused_input:        # (fp32 / fp16 plans pack their input: no whole-batch plans are built for nothing)
            return None
        pl = self._whole_batch_plans()[k]
        if not pl.fused_input or any(hd["op"] is None for hd in pl.heads) or pl.f32:
            return None
        self._make_nms_streams()
        self._fast_events = True                                  # (tests: the fast path was taken)
        return FastStep(self, k, pl, io, out, conf_thres, nms_thres)

    def detect_step(self, conf_thres, nms_thres):
        """The ``FastStep`` a lone ``detect()`` call uses (its own io / output buffers, made once per plan), or None.  One
        whole-batch list + NMS through one FFI call beats two joined half-batch lists for a host-synchronous call: SPP-640 x 32
        5.45 vs 5.87 ms, YOLOv3-tiny x 32 0.71 vs 0.90 ms (tools/detect_modes.py, three interleaved rounds on one box)."""
        fs = self._detect_fast
        if fs is None:
            from .utils.utils import nms_capacity
            with torch.cuda.device(self.device):
                cap = nms_capacity(self.rows_total, self.n_class)
                out = (torch.empty((self.bs, cap, 7), dtype=torch.float32, device=self.device),
                       torch.empty((self.bs, cap), dtype=torch.int32, device=self.device),
                       torch.empty((self.bs,), dtype=torch.int32, device=self.device))
                fs = self.fast_pipeline(0, None, out, conf_thres, nms_thres) or False      # (compact NMS form: no io)
            self._detect_fast = fs
        if fs is False:
            return None
        fs.step.conf_thres, fs.step.nms_thres = float(conf_thres), float(nms_thres)
        return fs

    def conv_flops(self) -> float:
        return sum(p.conv_flops() for p in self.subs)

    def activation_bytes(self) -> int:
        return sum(p.activation_bytes() for p in self.subs)

    def algorithmic_bytes(self, detect: bool = False) -> float:
        return sum(p.algorithmic_bytes(detect) for p in self.subs)


class FastStep:
    """One ring slot of ``detect_stream()``: a prebuilt ``YoloPipeStep`` (include/yolo_hip.h) - per batch the host patches the input
    pointer, records "x is ready" and makes ONE call into the library, which enqueues the layer list on the pipeline's stream, the
    NMS on the side stream, the count read-back into pinned memory and the events between them.  Slot and pipeline are tied
    (slot % S), so a slot's buffers are written by one pipeline only and its head launches wait for that pipeline's previous NMS."""

    def __init__(self, sp: "StreamedPlan", k: int, pl: Plan, io, out, conf_thres, nms_thres):
        from ._lib import YoloPipeStep
        from .utils.utils import MAX_PER_CLASS, MIN_WH
        self.sp, self.k, self.pl, self.io, self.out = sp, k, pl, io, out
        bs, rows, nc = sp.bs, pl.rows_total, pl.n_class
        self.compact = (torch.empty(K.nms_compact_workspace_bytes(bs, rows, nc), dtype=torch.uint8, device=sp.device), conf_thres,
                        MIN_WH) if io is None else None            # (a workspace per slot: two slots of a pipeline may be in flight)
        self.ws = self.compact[0] if io is None else torch.empty(K.nms_workspace_bytes(bs, rows, nc), dtype=torch.uint8, device=sp.device)
        self.count_host = torch.empty(bs, dtype=torch.int32).pin_memory()
        self.count_np = self.count_host.numpy()
        self.ready, self.done = K.Event(), K.Event()
        heads_done, nms_done = K.Event(), K.Event()              # per slot: the slot's head launches wait for the slot's previous NMS
        self._events = (heads_done, nms_done)
        self._launched = False
        fused = [hd["op"] for hd in pl.heads]
        st = YoloPipeStep()
        st.ops, st.n_ops, st.k_io = pl.op_array, pl.n_ops, min(fused)
        st.stream, st.nms_stream = sp.streams[k].cuda_stream, sp._nms_streams[k].cuda_stream
        st.wait_x, st.wait_io, st.heads_done, st.nms_done, st.done = self.ready.handle, None, heads_done.handle, nms_done.handle, self.done.handle
        st.io, st.bs, st.rows, st.nc, st.max_per_class = (None if io is None else io.data_ptr()), bs, rows, nc, MAX_PER_CLASS
        st.conf_thres, st.nms_thres, st.min_wh, st.cap = float(conf_thres), float(nms_thres), MIN_WH, out[0].shape[1]
        st.out_dets, st.out_idx, st.out_count = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
        st.workspace, st.workspace_bytes, st.count_host = self.ws.data_ptr(), self.ws.numel(), self.count_host.data_ptr()
        self.step = st
        self._nms_done = nms_done
        self._ps = tuple(None for _ in pl.heads)
        self._shape = tuple(pl.rec.input.buf.tensor.shape) if pl.rec.input.buf is not None and pl.rec.input.buf.tensor is not None else None
        self._x_shape = (pl.rec.c_in, pl.rec.input.h, pl.rec.input.w)

    def launch(self, x: torch.Tensor):
        """Enqueue one batch (no host sync).  ``x``: contiguous float32 NCHW of the planned shape on the plan's device."""
        pl, sp = self.pl, self.sp
        if x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape[1:]) != self._x_shape or x.shape[0] != sp.bs:
            raise RuntimeError("input must be contiguous float32 NCHW of the planned shape")
        pl.set_input_ptr(x.data_ptr())
        # (the plan may have served another caller's buffers in between, and detect() may change the threshold per call: Plan._bound
        # says what the head ops currently point at)
        if self.compact is not None:
            want = (self.compact[0].data_ptr(), float(self.step.conf_thres), self._ps)
            if pl._bound != want:
                self.compact = (self.compact[0], float(self.step.conf_thres), self.compact[2])
                pl._bind_outputs(None, self._ps, self.compact)
        elif pl._bound != (self.io.data_ptr(), None, self._ps):
            pl._bind_outputs(self.io, self._ps)
        # the whole-batch plans are shared with launch_detect's stream sets: same ordering rule as there
        if sp._full_mode:
            torch.cuda.synchronize(sp.device)
        sp._full_mode = False
        self.ready.record()                                     # on the caller's current stream: x was produced there
        # this slot's io was last read by the NMS of the slot's previous batch: the head launches wait for it
        self.step.wait_io = self._nms_done.handle if self._launched else None
        self._launched = True
        K.pipeline_step(self.step)

    def collect(self):
        """Wait for this slot's batch and hand out the reference's ``list[Tensor[n, 7] | None]``."""
        self.done.synchronize()
        counts = self.count_np.tolist()
        cap = self.out[0].shape[1]
        total = 0
        for b, n in enumerate(counts):
            if n > cap:
                raise RuntimeError(f"image {b}: {n} detections exceed the output capacity {cap}")
            total += n
        if total == 0:
            return [None] * len(counts)
        with torch.cuda.device(self.sp.device):                  # (the library launches on the CURRENT device's stream)
            packed = torch.empty((total, 7), dtype=torch.float32, device=self.sp.device)
            K.pack_detections(self.out[0], None, self.out[2], packed)
        parts = iter(torch.split(packed, [n for n in counts if n]))
        return [next(parts) if n else None for n in counts]


def _sym_to_nchw(s: Sym) -> torch.Tensor:
    t = s.buf.tensor[..., s.c_offset:s.c_offset + s.c]
    return t.permute(0, 3, 1, 2).float().contiguous()


def run_standalone(trace_fn, x: torch.Tensor):
    """Run a recorded sub-graph (a block, a stage) on an NCHW float32 CUDA tensor and return its
    output(s) as NCHW float32 — used by the block-level ``forward`` methods and their tests."""
    if not x.is_cuda:
        raise RuntimeError("pytorch_yolo_amd runs on a ROCm device only (no CPU fallback)")
    x = x.float().contiguous()
    bs, c, h, w = x.shape
    rec = Recorder(bs, c, h, w)
    out = trace_fn(rec, rec.input)
    with torch.cuda.device(x.device):               # the library launches on the current device's stream: make it x's
        plan = Plan(rec, x.device, n_class=0, img_size=max(h, w))
        plan.feed(x)
        K.run_ops(plan.op_array, plan.n_ops)
        if isinstance(out, (tuple, list)):
            return tuple(_sym_to_nchw(s) for s in out)
        return _sym_to_nchw(out)
