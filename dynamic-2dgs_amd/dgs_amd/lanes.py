"""Concurrent view lanes (Trainer(views_per_rank=k, concurrent_views=True)): the k views of a step in flight at the same time, each
on its own stream with its own alias modules, gradient bucket, rasterizer context and captured graph; one update behind them.

Mixin of dgs_amd.train.Trainer; a lane is a trainer of the same class (type(self)) that is used for its forward + backward only."""
import os

import torch

from .capture import StaticCamera


# per-instance scratch of the two model classes (streams, neighbour seeds, persistent tables, hooks): an alias starts without it
_ALIAS_SCRATCH = ("_side_stream", "_deferred", "_knn_seed", "_coherent_tables", "_g_attrs", "_pending_reduce", "_join_pending",
                  "_deferred_active", "view_select", "_graphed", "_graphed_keys", "_screenspace_leaf", "_before_sh_read")


def alias_module(m):
    """A module of the same class and configuration whose parameters are NEW Parameter objects over the SAME storage (values shared,
    an own .grad each) and whose buffers are the same tensors.  What a second view needs to run its forward and backward next to
    the first one's: the autograd leaves, the gradient sinks and every per-instance scratch buffer are its own; an in-place update
    or in-place surgery of the original is visible at once.  (Replacing a Parameter of the original breaks the alias: rebuild it.)"""
    import copy
    from collections import OrderedDict
    c = copy.copy(m)
    c.__dict__ = dict(m.__dict__)
    for k in _ALIAS_SCRATCH:
        c.__dict__.pop(k, None)
    c._parameters = OrderedDict((n, None if p is None else torch.nn.Parameter(p.data, requires_grad=p.requires_grad)) for n, p in m._parameters.items())
    c._buffers = OrderedDict(m._buffers)
    c._modules = OrderedDict((n, None if sub is None else alias_module(sub)) for n, sub in m._modules.items())
    return c


class LanesMixin:
    #   _lanes_built_for: _lanes_key() of the lanes in self._lanes; _stream0: lane 0's stream (lane 0 is the trainer itself)
    #   _lane_state: a lane between _lane_backward_to_surfels and _lane_backward_rest -- (render package, fused)
    #   _kloss: [1] loss of a k-view step, the mean of the views' losses (also the k-views-added path's accumulator)
    _lanes_built_for = _stream0 = _lane_state = _kloss = None
    #   _glanes: captured graphs of the lanes ([] in the one-graph form); None: the capture is not a lanes capture
    #   _gall: the one-graph form -- all lanes (single GPU: and the update) in one graph
    #   _overlap_was: deform.overlap_streams as _capture_lanes found it (enable_graph puts it back)
    _glanes = _gall = _overlap_was = None

    # ---- k views of a step in flight at the same time (concurrent_views) ---------------------------------------------------------
    def _concurrent(self):
        """Are the k views of a step run concurrently, a lane each?  The fully fused HIP path with the flat Adam kernel only."""
        s = self.surfels
        return bool(self.concurrent_views and self.views_per_rank > 1 and self._lane_of is None and self.rasterizer_cls is None
                    and self.opt_deform is None and s.get_xyz.is_cuda and self.fuse_deform and self.deform.can_assemble(s)
                    and not self._arap_active())

    def _lanes_key(self):
        """What the lanes were built for: the parameter storage they alias and the configuration they copied."""
        d, s = self.deform, self.surfels
        return (tuple(p.data_ptr() for p in self.bucket.params), self.views_per_rank, self.warmup, self.lambda_normal, self.lambda_dist,
                int(s.active_sh_degree), bool(getattr(d, "coherent_surfels", False)), getattr(d, "knn_refine_mode", None),
                bool(getattr(d, "fixed_point_tables", False)), bool(self.sh_grad_sink), bool(self.store_grads), self.P)

    def _make_lanes(self):
        """Lanes 1 .. k - 1: a Trainer each over ALIAS modules (alias_module: same parameter storage, own Parameter objects) with its
        own gradient bucket, rasterizer context and streams; used for _fwd_bwd only -- the optimiser, the statistics' accumulators,
        the step guard and the overflow flag are lane 0's (this trainer's).  Rebuilt whenever a parameter was replaced (growth, node
        densification) or the regime changed."""
        key = self._lanes_key()
        if self._lanes is not None and self._lanes_built_for == key:
            return self._lanes
        import diff_surfel_rasterization as dsr
        dev = self.surfels.get_xyz.device
        lanes = []
        for j in range(1, self.views_per_rank):
            sf, df = alias_module(self.surfels), alias_module(self.deform)
            ln = type(self)(sf, df, self.cameras, self.targets, self.bg, fused_adam=True, views_per_rank=self.views_per_rank, shard_optimizer=False)
            ln._lane_of, ln._lane = self, dsr.Lane(dev)
            ln._lane_index = j
            ln.rank, ln.world = self.rank, self.world
            ln.warmup, ln.lambda_normal, ln.lambda_dist = self.warmup, self.lambda_normal, self.lambda_dist
            ln.sh_grad_sink, ln.store_grads, ln.fuse_deform = self.sh_grad_sink, self.store_grads, self.fuse_deform
            ln._oflag = self._oflag          # ONE overflow flag for all lanes: any lane's overflow skips the step
            ln._stream = torch.cuda.Stream(dev, priority=int(os.environ.get("DGS_LANE_PRIORITY", "0")))
            ln._deterministic = self._deterministic
            if self._deterministic:
                ln._lane.context.set_option(7, 2)
                ln._lane.context.set_option(9, 0)
            lanes.append(ln)
        if self._stream0 is None:
            self._stream0 = torch.cuda.Stream(dev, priority=int(os.environ.get("DGS_LANE0_PRIORITY", "0")))
        self._lanes, self._lanes_built_for = lanes, key
        return lanes

    def _lane_list(self):
        """[(lane trainer, its stream)] of all k lanes, lane 0 = this trainer."""
        others = self._make_lanes()   # (also creates lane 0's stream)
        return [(self, self._stream0)] + [(ln, ln._stream) for ln in others]

    def _capture_lanes(self, dev):
        """One captured graph per lane -- view selection, deformation, render, loss, backward, the view's statistics -- on the lane's own
        stream and in a memory pool of its own (graphs that replay side by side must not share intermediates), and one graph for the
        update.  Replayed by _step_lanes."""
        k = self.views_per_rank
        lanes = self._lane_list()
        # no fork INSIDE a lane (one-view steps run the node MLP next to the neighbour search and its backward on a side stream): the other
        # lane is what fills the device here, and ROCm 7.2's graph instantiation segfaults on the nested forks of the one-graph form
        # (DGS_LANES_FLAT=0 with separate graphs works and measures the same: 0.650 / 0.657 ms per view)
        if os.environ.get("DGS_LANES_FLAT", "1") != "0":
            self._overlap_was = bool(self.deform.overlap_streams)   # lane 0 is this trainer's own module: enable_graph puts the switch back
            for ln, _ in lanes:
                ln.deform.overlap_streams = False
        for j, (ln, st) in enumerate(lanes):
            if ln is not self:   # the lane's own capture state: its row of the view table, its counters -- the big tables are shared
                ln._capacity, ln._list_hint = self._capacity, self._list_hint
                ln._ctx_option(2, self._capacity)
                ln._ctx_option(6, self._list_hint)
                ln._ctx_overflow_flag(self._oflag)
                ln._rays, ln._targets_c, ln._vtab = self._rays, self._targets_c, self._vtab
                ln._scam = StaticCamera(self.cameras[0], dev, self._rays[0][0], self._targets_c[0])
                ln._scam.load(self._vtab[0])
                ln._dev_select, ln._select_rider = self._dev_select, self._select_rider
                ln._new_view_counter(dev, self.iteration)
                ln._sgt = ln._scam.target
            ln._sel_stride, ln._sel_offset = k * self.world, j * self.world + self.rank   # view_for(i, j) = ((i k + j) world + rank) mod V
        self._vctr_host = int(self.iteration)
        cur = torch.cuda.current_stream()
        snap = self._snapshot()
        for _ in range(3):      # warm-up: allocations, lazily created per-lane buffers -- on a snapshot, nothing trains
            self._lanes_eager([(ln._scam, ln._sgt) for ln, _ in lanes])
            self._finish_lanes(eager=True)
        self._restore(snap)
        # (the captured update runs the optimiser over two parameter ranges: their block plans are built by a kernel on first use --
        # before the capture, not inside it)
        self.opt_surfels._range(0, self.n_surfel_params)
        self.opt_surfels._range(self.n_surfel_params, len(self.bucket.params))
        torch.cuda.synchronize()
        mode = {"capture_error_mode": "thread_local"}
        self._gall = None
        self._sloss = self._kloss     # (the warm-up steps created it; every replay rewrites it in place)
        self._gk = self._g1 = self._g1b = self._g0 = None
        one_graph = os.environ.get("DGS_LANES_ONE_GRAPH", "1" if self.world == 1 else "0") != "0" and os.environ.get("DGS_LANES_FLAT", "1") != "0"
        if one_graph:
            # ONE graph: the lanes fork from the capture stream and join in front of the update (single GPU: the update is part of
            # the graph) -- one replay per step, every lane starts at the same moment
            s0 = self._stream0
            s0.wait_stream(cur)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s0, **mode):
                for ln, st in lanes[1:]:
                    st.wait_stream(s0)
                # single GPU: the LAST lane (it starts last and ends last) stops behind its skinning backward -- every per-surfel gradient
                # of every lane is final there -- and the surfel update runs NEXT TO that lane's node-MLP backward chain, as in the
                # one-view step, instead of behind it (the update is 68 us of the step's serial tail otherwise)
                tail_overlap = self.world == 1 and os.environ.get("DGS_LANES_TAIL_OVERLAP", "1") != "0"
                last_ln, last_st = lanes[-1]
                for ln, st in lanes:
                    with torch.cuda.stream(st):
                        ln._select_view_node()
                        if tail_overlap and ln is last_ln:
                            ln._lane_loss = ln._lane_backward_to_surfels(ln._scam, ln._sgt)
                        else:
                            ln._lane_loss = ln._fwd_bwd(ln._scam, ln._sgt)
                        ln._select_consumed()
                for ln, st in lanes[1:]:
                    s0.wait_stream(st)
                if tail_overlap:
                    loss_first = os.environ.get("DGS_LANES_TAIL_ORDER", "mlp") == "loss"   # (A/B: 0.6250 loss first, 0.6234 chain first, 0.6308 without the overlap)
                    if loss_first:
                        self._lanes_loss()
                    if last_st is not s0:
                        last_st.wait_stream(s0)          # (the fork; lane 0 as the last lane cannot happen with k > 1)
                    with torch.cuda.stream(last_st):
                        last_ln._lane_backward_rest()    # node-MLP backward, weight gradients, this lane's statistics
                    if not loss_first:
                        self._lanes_loss()
                    self._finish_lanes(eager=False, join=last_st)
                else:
                    self._lanes_loss()
                    if self.world == 1:
                        self._finish_lanes(eager=False)
            cur.wait_stream(s0)
            self._gall = g
            self._glanes = []
            self._g2 = None
            if self.world > 1:
                self._g2 = torch.cuda.CUDAGraph()
                s = torch.cuda.Stream()
                s.wait_stream(cur)
                with torch.cuda.graph(self._g2, stream=s, **mode):
                    self._finish_lanes(eager=False)
                cur.wait_stream(s)
            return
        self._glanes = []
        for j, (ln, st) in enumerate(lanes):
            st.wait_stream(cur)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st, **mode):
                ln._select_view_node()
                ln._lane_loss = ln._fwd_bwd(ln._scam, ln._sgt)
                ln._select_consumed()
            self._glanes.append(g)
            cur.wait_stream(st)
        torch.cuda.synchronize()
        self._g2 = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(cur)
        with torch.cuda.graph(self._g2, stream=s, **mode):
            self._lanes_loss()
            self._finish_lanes(eager=False)
        cur.wait_stream(s)

    def _lane_backward_to_surfels(self, cam, gt):
        """_fwd_bwd of a lane up to the end of autograd's backward (rasterizer + skinning backward): all per-surfel gradients of the
        lane's bucket are final, the node-MLP backward is still to come (_lane_backward_rest)."""
        loss, pkg, asm, fused = self._forward(cam, gt)
        self._note_loss(loss.detach())
        self._run_backward(lambda: loss.backward(self._unit if fused else None), fused)
        self._lane_state = (pkg, fused)
        return loss.detach()

    def _lane_backward_rest(self):
        pkg, fused = self._lane_state
        self._lane_state = None
        d = self.deform
        if hasattr(d, "finish_backward") and not self.warmup:
            d.finish_backward(join=True)
        elif hasattr(d, "run_pending_reduce"):
            d.run_pending_reduce()
        self._statistics(pkg, fused)

    def _lanes_eager(self, cams):
        """The k lanes' forward + backward launched eagerly, each on its stream (the host issues them one after the other, the device
        overlaps them), joined on the current stream."""
        cur = torch.cuda.current_stream()
        lanes = self._lane_list()
        for (ln, st), (cam, gt) in zip(lanes, cams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                ln._lane_loss = ln._fwd_bwd(cam, gt)
        for ln, st in lanes:
            cur.wait_stream(st)
        self._lanes_loss()

    def _lanes_loss(self):
        """mean of the lanes' losses -> the step's loss (what the guard kernel reports)"""
        lanes = self._lane_list()
        if self._kloss is None:
            self._kloss = torch.zeros(1, dtype=torch.float32, device=self.bucket.flat.device)
        torch.mean(torch.stack([ln._lane_loss.reshape(()) for ln, _ in lanes]), dim=0, keepdim=True, out=self._kloss)
        self._note_loss(self._kloss)

    def _step_lanes(self, views):
        """Replay the k lane graphs side by side, then the update."""
        it = self.iteration - 1
        cur = torch.cuda.current_stream()
        lanes = self._lane_list()
        for j, ((ln, st), v) in enumerate(zip(lanes, views)):   # a lane's counter counts STEPS (its stride is k * world)
            self._aim_view(ln, it, v, self._scheduled_view(it, j))
        self._vctr_host = it + 1
        if self._gall is not None:
            self._gall.replay()
        else:
            for (ln, st), g in zip(lanes, self._glanes):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    g.replay()
            for ln, st in lanes:
                cur.wait_stream(st)
        if self.world > 1:
            self._lanes_fold()
            self._reduce()
        if self._g2 is not None:   # (one graph on a single GPU: the update is part of it)
            self._g2.replay()
        return self._kloss

    def _lanes_fold(self):
        """Data parallel: the exchange works on ONE bucket -- add the other lanes' gradients and statistics into lane 0's first."""
        for ln in self._make_lanes():
            self.bucket.flat.add_(ln.bucket.flat)
            torch.maximum(self._radii, ln._radii, out=self._radii)

    def _finish_lanes(self, eager, join=None):
        """Update behind the k concurrent lanes.  Single GPU: the lanes' buckets are summed by the Adam kernel itself (dgs_adam_step_sum2)
        and their statistics accumulated one after the other.  Data parallel: the other lanes are folded into lane 0's bucket first
        (the exchange works on one buffer) -- eagerly, in front of the all-reduce (`eager`; the captured update starts behind it).
        join: a stream on which the last lane's node-MLP backward is still running (_capture_lanes): the surfel parameters are
        updated next to it, the stream is joined, then the statistics and the deformation parameters follow."""
        if self.world > 1:
            if eager:
                self._lanes_fold()
                self._reduce()
            return self._finish(reduce=False)
        return self._finish(reduce=False, lanes=self._make_lanes(), join=join)

    def _multi_view_step_concurrent(self, views):
        """Eager twin of _step_lanes: the k views on their lanes' streams, one update."""
        self._lanes_eager([(self.cameras[v], self.targets[v % len(self.targets)]) for v in views])
        self._finish_lanes(eager=True)
        return self._kloss[0].detach().clone()
