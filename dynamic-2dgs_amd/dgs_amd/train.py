"""One training step of the hot path, view/timestamp-parallel over the GPUs of a node.

Compute of the reference's GUI.train_step (train_gui.py:272-313,372,410-432) in the iteration > 20000
regime (ARAP off, normal + distortion regularisers on): node deformation -> render (HIP rasterizer) ->
L1 + D-SSIM + normal + distortion loss -> backward -> [DP] one flat all-reduce -> Adam (surfels + deform).

Data parallelism (new design, the reference is single-process): every rank holds a full replica, renders its
own view of the step's batch, and all gradients live in ONE flat fp32 bucket that is all-reduced once per
step over RCCL/xGMI (backend "nccl"; "gloo" in the CPU tests) -- on the HIP path in two asynchronous slices that overlap the
rest of the backward and the SH update.  The bucket tail carries the densification
statistics (train_gui.py:411, gaussian_model.py:484-486) so replicas stay identical without a second sum.

This module holds the Trainer -- constructor, state, forward / backward, the update, the step -- and what other files import from it.
The rest of the class lives in one mixin per concern: guard.py (step guard, overflow recovery), capture.py (HIP-graph capture and
replay), exchange.py (the data-parallel exchange), lanes.py (concurrent view lanes), surgery.py (densification, reordering, growth).
"""
import os

import torch
import torch.distributed as dist

from . import losses as _losses
from . import trace
from .capture import CaptureMixin, StaticCamera  # noqa: F401  (StaticCamera, alias_module: imported from here by other files)
from .exchange import ExchangeMixin
from .guard import GuardMixin
from .lanes import LanesMixin, alias_module  # noqa: F401
from .losses import training_loss, training_loss_from_allmap
from .render import render
from .surgery import SurgeryMixin


class FlatGradBucket:
    """All gradients as views into one contiguous fp32 buffer (+ a tail of `extra` floats)."""

    def __init__(self, params, extra=0):
        self.params = [p for p in params if p.requires_grad]
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(n + extra, dtype=torch.float32, device=dev)
        self.n_grad = n
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.extra = self.flat[n:]

    def zero(self):
        self.flat.zero_()

    def all_reduce_mean(self, group=None, average=True):
        """average=False leaves the SUM in the bucket (the flat Adam kernel then reads grad / world itself)."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
            if average:
                self.flat[:self.n_grad].mul_(1.0 / dist.get_world_size(group))


def expon_lr(step, lr_init, lr_final, max_steps):
    """get_expon_lr_func (utils/general_utils.py:49-83) with lr_delay_steps = 0, the way the reference calls it."""
    import math
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    t = min(max(step / max_steps, 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


def split_step_allowed(world, overlap_allreduce, hip_fused_path, arap_active):
    """May the data-parallel step be split at the rasterizer inputs (backward half a | SH all-reduce | half b)?
    Half a differentiates the loss with respect to the ASSEMBLED rasterizer inputs only.  The ARAP regulariser reaches the
    deformation network directly (deform.network(...) inside arap_loss), not through those inputs, so while it is active the
    split would silently drop its gradient: the step then runs unsplit (one backward over everything, one all-reduce)."""
    return bool(world > 1 and overlap_allreduce and hip_fused_path and not arap_active)


class Trainer(GuardMixin, CaptureMixin, ExchangeMixin, LanesMixin, SurgeryMixin):
    # Learning rates of the reference's exponential schedules at the END of their decay (iteration >= 40000:
    # xyz 1.6e-6 * spatial_lr_scale, deform 1.6e-6; arguments/__init__.py:103-108, scene/deform_model.py:38,
    # utils/general_utils.py get_expon_lr_func), the other groups are constant in the reference.  With the
    # iteration-0 rates a fresh Adam moves every deform-head weight by 8e-4 in its first step, which on the
    # synthetic noise targets inflates d_scaling to 4x the surfel scale after ONE step (mean radius 20 -> 75 px,
    # num_rendered x14): the timed workload would no longer be the 200k-surfel scene the metric names.
    LATE_POSITION_LR = 0.0000016
    LATE_DEFORM_LR = 0.0000016
    # lr_schedule=True: the reference's schedules from iteration 0 instead (arguments/__init__.py:104-108,126):
    #   xyz: 1.6e-4 -> 1.6e-6 (x spatial_lr_scale 5) over 30000 steps (gaussian_model.py:203-212);
    #   deformation network: 1.6e-4 * 5 -> 1.6e-6 over 40000 steps; the 'nodes' group STAYS at 1.6e-4 * 5 -- the reference's
    #   update_learning_rate returns after the first matching group (scene/deform_model.py:58-63).
    # On the HIP path the schedule is evaluated inside the Adam kernel from the device step counter (no host update, the
    # captured graph stays valid); on the CPU path the group rates are set before each optimiser step.
    SCHED_POSITION = (0.00016, 0.0000016, 30_000)
    SCHED_DEFORM = (0.00016 * 5, 0.0000016, 40_000)
    # State that is created on first use (the mixins declare theirs the same way): the defaults say "not there yet".
    #   opt_surfels, opt_deform: _build_state -- FlatAdam + None (HIP path), or two torch.optim.Adam
    #   _store_key: what _store_ok's cached verdict (_store_val) was computed for; _unit: dL/dloss = 1 of the fused path's backward
    #   _late_stats: (pkg, fused) of statistics that _finish launches behind the surfel update
    #   _half: split step, between half a and half b -- (assembled inputs, their gradients, render package)
    #   _kx, _kr: k views added -- sum / max of the views' statistics (_stats_accumulate); _arap_gen: generator of the ARAP term's random times
    opt_surfels = opt_deform = _store_key = _unit = _late_stats = _half = _kx = _kr = _arap_gen = None
    #   _bucket_clean: the last update cleared the gradients behind its reads (FlatAdam.zero_grads)
    #   _store_now: the step being built stores its gradients, no fill of the bucket (_forward_head)
    #   _guard_early: the guard kernel of the step rode in its loss node (_forward)
    _bucket_clean = _store_now = _guard_early = False
    _accum_view = 0                   # j > 0 while view j of a k-views-added step is built: producers add

    def __init__(self, surfels, deform, cameras, targets, bg_color, deform_lr=LATE_DEFORM_LR, position_lr=LATE_POSITION_LR,
                 fused_adam=None, rasterizer_cls=None, lr_schedule=False, arap=False, views_per_rank=1, shard_optimizer=True,
                 concurrent_views=False, alpha_masks=None, mask_as_scene=False, mask_as_dynamic=False, random_bg_color=False,
                 white_background=False):
        self.surfels, self.deform = surfels, deform
        # The ground-truth alpha masks of the views and what the reference does with them (all off by default there as well:
        # arguments/__init__.py:99,147-148; train_gui.py:287,302-311,365-369):
        #   mask_as_scene (gt_alpha_mask_as_scene_mask): the target is composited over the render's background -- a fresh random one per
        #     step with random_bg_color on a black-background scene, the white background otherwise -- so that nothing outside the mask is fitted;
        #   mask_as_dynamic (gt_alpha_mask_as_dynamic_mask): the surfels' motion mask (SurfelModel(with_motion_mask=True)) is rendered
        #     with everything else detached and pulled towards the mask, weight 0.5 -> 0.01 over the first 10 000 iterations, then 0.
        # While one of these terms is active the step runs on the unfused eager path (PyTorch loss, a second render), like the ARAP term.
        self.alpha_masks = None if alpha_masks is None else list(alpha_masks)
        self.mask_as_scene, self.mask_as_dynamic = bool(mask_as_scene), bool(mask_as_dynamic)
        self.random_bg_color, self.white_background = bool(random_bg_color), bool(white_background)
        self.bg_draw = None      # optional callable -> [3] background (tests replay the reference's draws); None: torch.rand_like
        self._mask_of = {} if alpha_masks is None else {id(t): m for t, m in zip(targets, self.alpha_masks)}
        # views_per_rank = k > 1 with concurrent_views: the k views of a step are IN FLIGHT AT THE SAME TIME, each on its own stream --
        # 55 % of a view's step are short launches that leave most of the device idle, and the two blend kernels issue at half the
        # VALU rate; another view's work fills both.  Every view is a LANE: alias modules over the same parameter storage (own autograd
        # leaves, own scratch), an own gradient bucket (every producer STORES, as in a one-view step: nothing adds into a shared
        # buffer, so nothing races), an own library context of the rasterizer (diff_surfel_rasterization.Lane), an own captured graph.
        # The update reads the sum of the buckets on the fly (dgs_adam_step_sum2); see _make_lanes / _capture_lanes / _step_lanes.
        self.concurrent_views = bool(concurrent_views)
        self._lane = None        # this trainer's own diff_surfel_rasterization.Lane when it IS a lane of another trainer (else the default context)
        self._lanes = None       # lanes 1 .. k - 1 (Trainer objects over alias modules); lane 0 is this trainer itself
        self._lane_of = None
        # Data parallel (N > 1), split step: the SH coefficients -- 2/3 of the bucket -- are updated by the rank that OWNS their rows
        # (contiguous slot range rank * P / N ...): reduce-scatter of the SH gradients instead of their all-reduce, Adam on P / N rows
        # instead of P (the update is HBM-bound and was replicated on every rank), all-gather of the updated rows IN PLACE into the
        # parameter -- the same bytes on the wire as the all-reduce, but the second half of them (the all-gather) is only needed by
        # the NEXT step's preprocess kernel and rides under that step's deformation head (_shard_ok, _gather_sh_start).  No change of
        # the numerics: every element sees the same sum and the same update, from one rank instead of N.  The SH moments of rows a
        # rank does not own go stale there; whoever reads moments across rows (densification, reordering, growth) goes through
        # _moments(), which gathers them first.
        self.shard_optimizer = bool(shard_optimizer)
        self._ag_work = None            # the all-gather of the last step's SH update, waited for where the next reader of SH starts
        surfels.__dict__["_before_sh_read"] = self._wait_gather   # ... including readers outside the trainer (SurfelModel._settle_sh)
        self._sh_moments_local = False  # True: only this rank's rows of the SH moments are current
        # k > 1 (opt-in, data parallelism): every rank renders k views per step and ADDS their gradients before the one exchange of the
        # step -- neighbour search, the all-reduces and the Adam update once per k views instead of once per view; a step then trains on
        # k * world views (gradient = their mean), `iteration` counts steps.  See _multi_view_step.
        self.views_per_rank = int(views_per_rank)
        assert self.views_per_rank >= 1
        # ARAP regulariser of the control nodes with the reference's weight schedule (dgs_amd/arap.py; non-zero for
        # iterations < 20000).  Eager only: it draws random times and runs a batched SVD, neither belongs in a captured step.
        self.arap = bool(arap)
        self.arap_from = 0   # first iteration that adds it (the reference: after opt.warm_up = 3000, train_gui.py:315)
        self.lr_schedule = bool(lr_schedule)
        if lr_schedule:
            position_lr, deform_lr = self.SCHED_POSITION[0], self.SCHED_DEFORM[0]
        self._steps_done = 0
        self._adopted_steps = {}   # bucket index -> steps an adopted optimiser had taken (adopt_deform_state; used by set_regime)
        self.rasterizer_cls = rasterizer_cls  # None = the HIP operator; tests / the CPU baseline inject the oracle op
        self.cameras, self.targets, self.bg = cameras, targets, bg_color
        self._lrs = (position_lr, deform_lr)
        dev = surfels.get_xyz.device
        self.fused_adam = dev.type == "cuda" if fused_adam is None else fused_adam
        self._build_state()
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.iteration = 0
        self._graph = None
        self.overlap_allreduce = True  # DP: all-reduce the SH gradients while the deformation backward runs
        # DP, third split (off by default until an N > 1 RCCL run says it pays): the per-surfel non-SH gradients (xyz, scaling,
        # rotation, opacity, feature: 18 floats per surfel) are final after the skinning backward and start their all-reduce
        # there, under the node-MLP backward + weight gradients; only the deformation parameters and the statistics wait for
        # the end of the backward.  Costs two more graph replays per step.
        self.split3 = False
        # diagnostic (bench.py's `comm` object): True makes every collective of the step a no-op, so that a window of steps timed
        # with it shows what the step costs WITHOUT communication (the replicas diverge: callers restore a snapshot afterwards)
        self.no_collectives = False
        # Lever for links that deliver less than the plan needs: the two big slices of the split step -- the SH
        # gradients and, with split3, the per-surfel gradients -- cross the wire as bfloat16 (half the bytes: 57.7 -> 38.5 MB per step
        # at 200k surfels) and come back into the fp32 bucket.  A DELIBERATE change of the training numerics (8 mantissa bits on the
        # summed gradient of these slices; Adam normalises the scale away), off by default; every rank receives the same reduced
        # values, so the replicas stay bit-identical.  The deformation parameters, the densification statistics and the radii stay
        # fp32 / int32.  DGS_WIRE_BF16=1 switches it on in bench.py.
        self.wire_bf16 = os.environ.get("DGS_WIRE_BF16", "0") == "1"
        self.sh_grad_sink = True  # packed SH on HIP: no separate dL/dSH buffer, no accumulate pass
        self.store_grads = os.environ.get("DGS_STORE_GRADS", "1") != "0"   # fused path: gradients are stored, the bucket is never cleared (_store_ok)
        self.fuse_deform = True  # HIP: KNN + node MLP + skinning + surfel activations as fused kernels (ControlNodes.forward_assembled)
        # Regime of the reference step (train_gui.py:282-285,292-293).  Defaults = its late regime (iteration > 8000), which is what
        # the benchmark times; fit() walks through the schedule with set_regime():
        #   warmup (iteration < opt.warm_up = 3000): the deformation is applied but DETACHED -- nothing behind d_xyz / d_rotation /
        #     d_scaling receives a gradient: the node parameters, the network and the surfels' hyper coordinates stay untouched;
        #   lambda_normal / lambda_dist: 0 until iteration 8000, then 0.02 / 1000.
        self.warmup = False
        self.lambda_normal, self.lambda_dist = 0.02, 1000.0
        # step guard (capacity mode): see _init_guard / _check_guard
        self._guard_steps = 0
        self._guard_events = {}
        self._skipped_seen = 0
        self.overflow_recoveries = 0

    def _build_state(self):
        """Flat gradient bucket + optimiser over the current parameter tensors (again after Trainer.grow)."""
        surfels, deform = self.surfels, self.deform
        position_lr, deform_lr = self._lrs
        P = surfels.get_xyz.shape[0]
        self.P = P
        surf_params = [p for g in surfels.optimizer_groups() for p in g['params']]
        if getattr(surfels, "packed_sh", False):
            # the SH gradient (2/3 of the bucket) first: under data parallelism it is final right after the rasterizer's
            # backward and is all-reduced while the rest of the backward still runs (see step())
            surf_params = [surfels._features] + [p for p in surf_params if p is not surfels._features]
        params = surf_params + list(deform.parameters())
        self.bucket = FlatGradBucket(params, extra=2 * P)
        self.n_sh = surfels._features.numel() if getattr(surfels, "packed_sh", False) else 0
        dev = surfels.get_xyz.device
        fused_adam = self.fused_adam
        groups = surfels.optimizer_groups(position_lr=position_lr)
        deform_groups = [
            {'params': list(deform.network.parameters()), 'lr': deform_lr, 'name': 'deform'},
            {'params': [deform.nodes, deform._node_radius, deform._node_weight], 'lr': deform_lr, 'name': 'nodes'}]
        self.n_surfel_params = sum(len(g['params']) for g in surfels.optimizer_groups())
        if dev.type == "cuda" and hasattr(deform, "grad_sink"):
            deform.grad_sink = True  # the fused node MLP adds its weight gradients straight into the bucket views
            # ... and its backward is launched by _fwd_bwd on a side stream, next to the surfels' Adam update
            deform.defer_mlp_backward = fused_adam
        if fused_adam:
            # HIP device: one flat Adam launch for surfels + deformation (csrc/step_kernels.h); step counter on the device
            from . import _ops
            lr_of = {id(p): g['lr'] for g in groups + deform_groups for p in g['params']}
            pat_of = {id(p): g['pattern'] for g in groups for p in g['params'] if 'pattern' in g}
            plist = self.bucket.params  # bucket order == layout of the flat gradient buffer
            patterns = {i: pat_of[id(p)] for i, p in enumerate(plist) if id(p) in pat_of}
            schedules = {}
            if self.lr_schedule:
                net = {id(p) for p in deform.network.parameters()}
                scale = groups[0]['lr'] / position_lr   # spatial_lr_scale, applied by optimizer_groups
                for i, p in enumerate(plist):
                    if p is surfels._xyz:
                        schedules[i] = (self.SCHED_POSITION[1] * scale, self.SCHED_POSITION[2])
                    elif id(p) in net:
                        schedules[i] = (self.SCHED_DEFORM[1], self.SCHED_DEFORM[2])
            old = self.opt_surfels
            self.opt_surfels = _ops.FlatAdam(plist, [lr_of[id(p)] for p in plist], self.bucket.flat, patterns=patterns,
                                             schedules=schedules, sched_t0=float(self._steps_done))
            self.opt_deform = None
            if old is not None and hasattr(old, "_origin"):
                # rebuilt state (grow / node densification): the parameters keep their step origins -- by position when the list is
                # the same length (a rebuild replaces the tensors), by identity for whatever survives a changed list
                if len(old._origin) == len(plist):
                    for i in range(len(plist)):
                        self.opt_surfels._origin[i] = old._origin[i]
                else:
                    was = {id(p): old._origin[i] for i, p in enumerate(getattr(old, "params", []))}
                    for i, p in enumerate(plist):
                        if id(p) in was:
                            self.opt_surfels._origin[i] = was[id(p)]
            self.opt_surfels.zero_grads = False  # True: step + zero_grad in one pass, see _forward for why it is off
            self._bucket_clean = False
            self._init_guard(old)
        else:
            assert not getattr(surfels, "packed_sh", False), "packed SH needs the flat Adam kernel (two rates inside one parameter)"
            self.opt_surfels = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
            self._spatial = groups[0]['lr'] / position_lr
            if self.opt_deform is None:   # kept across Trainer.grow: the deformation parameters do not move
                self.opt_deform = torch.optim.Adam(deform_groups, lr=0.0, eps=1e-15)

    def _forward_head(self, cam):
        """The forward in FRONT of the rasterizer: gradient-bucket handling and the deformation (neighbour search, node MLP, skinning,
        surfel activations).  Reads every parameter except the SH coefficients -- which is why the sharded data-parallel step runs it
        while the all-gather of the previous step's SH update is still on the wire (_gather_sh_start)."""
        s, d = self.surfels, self.deform
        # The gradient bucket (57 MB) is cleared by a fill in front of the step (10 us).  Two alternatives were built and measured
        # on the replayed step: (a) the flat Adam kernel clears the gradients behind its reads (FlatAdam.zero_grads; the bucket
        # is then clean after every complete update and no fill is launched: _bucket_clean, host state evaluated when a step is
        # BUILT) -- but the 57 MB of extra writes land in the SH update, the longer branch of the step's tail (84 -> 101 us);
        # (b) the fill on its own stream next to the neighbour search, joined before the backward -- a cross-stream dependency
        # inside a replayed graph costs 5-10 us of idle device at the fork AND at the join, more than the fill.
        # (c, round 3, what runs now) NO fill: on the fully fused path every element of the bucket is STORED by the kernel that
        # produces it in every step (dL/dSH with zeros for culled rows: rasterizer option 8; the skinning backward, its node-table
        # reduction and the node MLP's weight gradients in overwrite mode; the statistics), so nothing needs clearing (_store_ok).
        t = d.expand_time(cam.fid)
        fused = self.rasterizer_cls is None and s.get_xyz.is_cuda and not self._mask_terms()
        assemble = fused and self.fuse_deform and d.can_assemble(s)
        adding = self._accum_view > 0   # view 2 .. k of a multi-view step: every producer ADDS to what the earlier views left
        self._store_now = bool(assemble and torch.is_grad_enabled() and self._store_ok()) and not adding
        if hasattr(d, "grad_sink") and d.grad_sink:
            d.grad_sink = "store" if self._store_now else True
        if not adding and not self._store_now and not (self._bucket_clean and self.opt_deform is None and self.opt_surfels.zero_grads):
            self.bucket.zero()
        if hasattr(d, "reuse_knn"):
            d.reuse_knn = adding             # the surfels and nodes have not moved since the step's first view: its neighbours stand
        self._bucket_clean = False
        asm = dv = None
        if assemble:
            with trace.stage("dgs.deform"):
                asm = d.forward_assembled(s, t)
        else:
            dv = d(s.get_xyz.detach(), t, s.feature, s.motion_mask)
            if self.warmup:
                dv = {k: v.detach() for k, v in dv.items()}
        return asm, dv, fused

    def _forward(self, cam, gt, head=None):
        """head: what _forward_head returned for this view when the caller ran it separately (sharded data-parallel step)."""
        s = self.surfels
        gt0 = gt
        asm, dv, fused = self._forward_head(cam) if head is None else head
        if asm is not None:
            with trace.stage("dgs.rasterize"):
                pkg = render(cam, s, self.bg, rasterizer_cls=self._raster_cls(), postprocess=False, assembled=asm)
        else:
            mask = self._mask_of.get(id(gt)) if self._mask_of else None
            random_bg = bool(mask is not None and self.mask_as_scene and self.random_bg_color and not self.white_background)   # train_gui.py:287
            if random_bg:
                random_bg = self.bg_draw() if self.bg_draw is not None else True
            pkg = render(cam, s, self.bg, dv['d_xyz'], dv['d_rotation'], dv['d_scaling'], rasterizer_cls=self._raster_cls(),
                         postprocess=not fused, random_bg_color=random_bg)
            if mask is not None and random_bg is not False:                                      # train_gui.py:302-307
                gt = mask * gt + (1 - mask) * pkg["bg_color"][:, None, None]
            elif mask is not None and self.white_background and self.mask_as_scene:
                gt = mask * gt + (1 - mask) * self.bg[:, None, None]
        lam = dict(lambda_normal=self.lambda_normal, lambda_dist=self.lambda_dist)
        # unit_grad: every backward of this trainer starts from dL/dloss = 1 (self._unit; the ARAP term is added, not multiplied), so
        # the loss node produces its gradient images in the forward (regularisers: value and gradient in one kernel)
        # single GPU: the step guard rides in the loss node (the thread that writes the loss runs it): everything it reads exists
        # then, and the surfels' Adam update later starts right behind the skinning backward (_finish: advance=False)
        ride = (fused and torch.is_grad_enabled() and self.world == 1 and self.opt_deform is None and self._oflag is not None
                and not self._arap_active() and _losses.FUSE_PHOTOMETRIC and self.views_per_rank == 1)
        with trace.stage("dgs.loss"):
            loss = (training_loss_from_allmap(pkg["render"], pkg["allmap"], cam, gt, unit_grad=True, guard=self.opt_surfels if ride else None, **lam)
                    if fused else training_loss(pkg, gt, **lam))
        self._guard_early = bool(ride)
        lam_motion = self._lambda_motion_mask()
        if asm is None and lam_motion > 0 and self._mask_of.get(id(gt0)) is not None:              # train_gui.py:363-369
            mask = self._mask_of[id(gt0)]
            random_bg = bool(self.mask_as_scene and self.random_bg_color and not self.white_background)
            if random_bg:
                random_bg = self.bg_draw() if self.bg_draw is not None else True
            motion = render(cam, s, self.bg, dv['d_xyz'], dv['d_rotation'], dv['d_scaling'], rasterizer_cls=self._raster_cls(), postprocess=False,
                            random_bg_color=random_bg, render_motion=True, detach_xyz=True, detach_rot=True, detach_scale=True, detach_opacity=True)
            loss = loss + lam_motion * torch.abs(mask - motion["render"][0]).mean()
        if self.arap:
            from . import arap
            lam = arap.lambda_arap(self.iteration)       # train_gui.py:315-316, utils/time_utils.py:1228-1232
            if lam > 0 and self.iteration > self.arap_from:
                if self._arap_gen is None:
                    self._arap_gen = torch.Generator(device=s.get_xyz.device).manual_seed(1234 + self.rank)
                loss = loss + lam * arap.arap_loss(self.deform, generator=self._arap_gen)
        if fused and self._unit is None:
            self._unit = torch.ones((), dtype=loss.dtype, device=loss.device)
        return loss, pkg, asm, fused

    MOTION_MASK_LANDMARKS, MOTION_MASK_STEPS = (5e-1, 1e-2, 0), (0, 10_000, 10_001)     # arguments/__init__.py:143-144

    def _lambda_motion_mask(self):
        if not (self.mask_as_dynamic and self._mask_of):
            return 0.0
        from .arap import landmark_interpolate
        return landmark_interpolate(self.MOTION_MASK_LANDMARKS, self.MOTION_MASK_STEPS, self.iteration)

    def _mask_terms(self):
        """True while a term that needs the ground-truth masks is part of the step being built (the unfused eager path serves them)."""
        if not self._mask_of:
            return False
        scene = self.mask_as_scene and (self.white_background or self.random_bg_color)
        return bool(scene or self._lambda_motion_mask() > 0)

    def _store_ok(self):
        """May this step run without clearing the gradient bucket?  Only if EVERY parameter in it has a producer that overwrites
        (see _forward): packed SH through the sink, the five per-surfel parameters and the three node tensors through the fused
        skinning backward, the node MLP's weights through its deferred backward -- and nothing adds to a .grad through autograd
        (the ARAP term does)."""
        if not self.store_grads or self.opt_deform is not None or self._arap_active():
            return False
        s, d = self.surfels, self.deform
        # everything the verdict depends on is in the key: the bucket and optimiser objects themselves (kept alive by the key, so an
        # id cannot be reused), and the public switches a caller may flip between steps
        key = (self.bucket, self.opt_surfels, s.feature.shape[1], bool(self.sh_grad_sink), bool(getattr(d, "defer_mlp_backward", False)),
               bool(getattr(d, "grad_sink", False)), bool(getattr(d, "overlap_streams", False)))
        old = self._store_key
        if old is None or len(old) != len(key) or any(a is not b and a != b for a, b in zip(old, key)):
            ok = (getattr(s, "packed_sh", False) and self.sh_grad_sink and self.n_sh > 0 and getattr(d, "defer_mlp_backward", False)
                  and bool(getattr(d, "grad_sink", False)) and s.feature.shape[1] == d.hyper_dim)
            if ok:
                from . import _ops
                mlp = _ops.node_mlp_params(d.network) or []
                covered = {id(p) for p in (s._features, s._xyz, s._scaling, s._rotation, s._opacity, s.feature, d.nodes, d._node_radius,
                                           d._node_weight)} | {id(p) for p in mlp}
                ok = bool(mlp) and all(id(p) in covered for p in self.bucket.params)
            self._store_key, self._store_val = key, bool(ok)
        return self._store_val

    def _run_backward(self, fn, fused):
        """fn() under the SH gradient sink when it applies (the rasterizer's backward then writes dL/dSH straight into the
        bucket view of the packed parameter)."""
        s = self.surfels
        # (views 2 .. k of a multi-view step: the sink STORES the rows of the visible surfels, it does not add to them -- those views
        # take the operator's own dL/dSH tensor and autograd adds it to the bucket view: one 4 P M-byte pass more per extra view)
        if fused and getattr(s, "packed_sh", False) and self.sh_grad_sink and not self._accum_view and self._lane is not None:
            # a lane's sink is a field of its own Lane object: nothing device-wide, nothing keyed by the (shared) parameter storage
            self._lane.sink, self._lane.all_rows = s._features.grad, bool(self._store_now)
            try:
                return fn()
            finally:
                self._lane.sink = None
        if fused and getattr(s, "packed_sh", False) and self.sh_grad_sink and not self._accum_view:
            import diff_surfel_rasterization as dsr
            # the sink belongs to THIS trainer's SH parameter (keyed by the tensor the forward was given): other trainers on the
            # device keep theirs, and removing it afterwards removes nothing else
            dsr.set_sh_grad_sink(s._features.grad, all_rows=self._store_now, shs=s._features)
            try:
                return fn()
            finally:
                dsr.set_sh_grad_sink(None, shs=s._features)
        return fn()

    def _raster_cls(self):
        """What render() instantiates: the injected operator (tests, CPU baseline), the HIP operator in this trainer's lane, or None
        (= the HIP operator in the device's default context)."""
        if self.rasterizer_cls is not None or self._lane is None:
            return self.rasterizer_cls
        import functools
        from diff_surfel_rasterization import GaussianRasterizer
        return functools.partial(GaussianRasterizer, lane=self._lane)

    def _statistics(self, pkg, fused, early_radii=False):
        with torch.no_grad():
            # densification statistics of this view into the bucket tail (summed over ranks)
            if self._radii is None:
                self._radii = torch.zeros(self.P + 4, dtype=pkg["radii"].dtype, device=pkg["radii"].device)
            if fused:
                from . import _ops
                radii_vis = self._radii
                if early_radii:   # split step: radii + flag were copied (and their all-reduce started) right after the forward
                    if self._radii_scratch is None:
                        self._radii_scratch = torch.empty_like(self._radii)
                    radii_vis = self._radii_scratch
                elif self.world > 1 and self._oflag is not None:
                    self._radii[self.P:self.P + 1].copy_(self._oflag)
                _ops.densify_view(pkg["radii"], pkg["viewspace_points"].grad, self.bucket.extra[:self.P], self.bucket.extra[self.P:2 * self.P],
                                  radii_vis)
            else:
                vis = pkg["visibility_filter"]
                g2 = pkg["viewspace_points"].grad[:, :2].norm(dim=-1)
                self.bucket.extra[:self.P].copy_(torch.where(vis, g2, torch.zeros_like(g2)))
                self.bucket.extra[self.P:2 * self.P].copy_(vis.to(torch.float32))
                self._radii[:self.P].copy_(torch.where(vis, pkg["radii"], torch.zeros_like(pkg["radii"])))

    def _note_loss(self, loss):
        """The guard kernel of this step copies the loss into its report (FlatAdam.loss)."""
        if self.opt_deform is None:
            self.opt_surfels.loss = loss.reshape(1)

    def _fwd_bwd(self, cam, gt):
        d = self.deform
        loss, pkg, asm, fused = self._forward(cam, gt)
        self._note_loss(loss.detach())
        # explicit unit gradient: loss.backward() alone launches a fill for it every step
        with trace.stage("dgs.backward"):
            self._run_backward(lambda: loss.backward(self._unit if fused else None), fused)
        if hasattr(d, "finish_backward") and not self.warmup:   # (warm-up: nothing behind the deformation's outputs trains)
            # single GPU, one view per step: joined inside _finish
            d.finish_backward(join=self.world > 1 or self.opt_deform is not None or self.views_per_rank > 1)
        elif hasattr(d, "run_pending_reduce"):
            d.run_pending_reduce()
        if getattr(d, "_join_pending", False) and fused:
            # single GPU: the node-MLP backward now runs on the side stream and is the longer branch; the statistics kernels
            # (three launches, ~25 us of a mostly idle device) go behind the surfel update instead of in front of it (_finish)
            self._late_stats = (pkg, fused)
        else:
            self._statistics(pkg, fused)
        return loss.detach()

    # ---- data parallel: the backward in two halves with the SH all-reduce in between ---------------------------------
    def _arap_active(self):
        """True while the ARAP term is part of the loss of the step being built (same test as _forward)."""
        if not self.arap:
            return False
        from .arap import lambda_arap
        return lambda_arap(self.iteration) > 0 and self.iteration > self.arap_from

    def _split_ok(self):
        s = self.surfels
        hip_fused = (self.rasterizer_cls is None and s.get_xyz.is_cuda and self.fuse_deform and getattr(s, "packed_sh", False)
                     and self.sh_grad_sink and self.n_sh > 0 and self.deform.can_assemble(s))
        return self.views_per_rank == 1 and split_step_allowed(self.world, self.overlap_allreduce, hip_fused, self._arap_active())

    def _fwd_bwd_a(self, cam, gt, head=None):
        """Forward, loss and the backward down to the rasterizer's inputs: afterwards the SH segment of the bucket is final."""
        loss, pkg, asm, fused = self._forward(cam, gt, head)
        leaf = pkg["viewspace_points"]
        grads = self._run_backward(lambda: torch.autograd.grad(loss, list(asm) + [leaf], grad_outputs=self._unit, allow_unused=True), fused)
        leaf.grad = grads[4]
        self._note_loss(loss.detach())
        self._half = (asm, grads[:4], pkg)
        with torch.no_grad():   # final after the forward: their MAX all-reduce starts first (the guard of the SH update needs it)
            # radii (0 for culled surfels: same as the masked copy of _statistics) + the overflow flag behind them, in ONE launch (two
            # copies were two 4-us launches with a gap between them on the boundary between graph 1 and graph 1b)
            torch.cat((pkg["radii"], self._oflag), out=self._radii[:self.P + 1])
        return loss.detach()

    def _fwd_bwd_b(self):
        """The rest of the backward: skinning / activations, node MLP, statistics."""
        self._fwd_bwd_b1()
        self._fwd_bwd_b2()

    def _fwd_bwd_b1(self):
        """Skinning / activation backward: afterwards every per-surfel gradient is final (second bucket segment)."""
        asm, g_asm, pkg = self._half
        keep = [(a, g) for a, g in zip(asm, g_asm) if g is not None]
        torch.autograd.backward([a for a, _ in keep], [g for _, g in keep])

    def _fwd_bwd_b2(self):
        """Node-MLP backward + weight gradients, statistics: the deformation parameters and the bucket tail are final."""
        _, _, pkg = self._half
        if not self.warmup:
            self.deform.finish_backward(join=True)
        elif hasattr(self.deform, "run_pending_reduce"):
            self.deform.run_pending_reduce()
        self._statistics(pkg, True, early_radii=True)
        self._half = None

    def _accumulate_stats(self, lanes=()):
        """The densification statistics of the step's view(s) -- bucket tail and radii -- into the surfels' accumulators."""
        s = self.surfels
        if self.rasterizer_cls is None and s.get_xyz.is_cuda:
            from . import _ops
            for tr in (self,) + tuple(lanes):   # every lane's view statistics (add_densification_stats once per view, gaussian_model.py:484-486)
                _ops.densify_accumulate(tr.bucket.extra[:self.P], tr.bucket.extra[self.P:2 * self.P], tr._radii[:self.P],
                                        s.xyz_gradient_accum, s.denom, s.max_radii2D,
                                        skip=self.opt_surfels.skip if self.opt_deform is None else None)
        else:
            s.xyz_gradient_accum.add_(self.bucket.extra[:self.P, None])
            s.denom.add_(self.bucket.extra[self.P:2 * self.P, None])
            torch.maximum(s.max_radii2D, self._radii[:self.P], out=s.max_radii2D)

    def _finish(self, reduce=True, sh_done=False, mid_done=False, lanes=(), join=None):
        """What follows a step's backward: the exchange (unless the caller ran it), the gradient scale, the statistics and the Adam
        update -- torch.optim.Adam on the CPU path (_update_torch), the flat kernel on the HIP path (_update_flat)."""
        s = self.surfels
        with torch.no_grad():
            if reduce:
                self._reduce()
            k = self.views_per_rank
            if self.opt_deform is None:
                self.opt_surfels.grad_scale = (1.0 / self.world if self._fold_mean else 1.0) / k
            elif k > 1:
                self.bucket.flat[:self.bucket.n_grad].mul_(1.0 / k)   # (torch.optim.Adam path: the bucket holds the mean over the ranks of the SUM over the k views)
            if lanes:   # concurrent views on one GPU: lane 1's bucket is the update's second gradient buffer, further lanes are added into it
                for ln in lanes[1:]:
                    lanes[0].bucket.flat.add_(ln.bucket.flat)
                self.opt_surfels.grad2 = lanes[0].bucket.flat
            late, self._late_stats = self._late_stats, None
            adv = not self._guard_early   # the guard kernel of this step was launched by _fwd_bwd already
            self._guard_early = False
            if late is None and join is None:
                self._accumulate_stats(lanes)
            # warm-up: everything up to (not including) `feature` -- unless the motion-mask term is on: its render reaches the mask column
            # of `feature` whether or not the deformation is detached (the hyper columns then see a zero gradient: Adam leaves them)
            feature_idle = self.warmup and not (self._lambda_motion_mask() > 0 and getattr(s, "with_motion_mask", False))
            if self.opt_deform is not None:
                self._update_torch(feature_idle)
            else:
                self._update_flat(self.n_surfel_params - 1 if feature_idle else None, adv, late, sh_done, mid_done, lanes, join)
            # every branch ran the update over ALL parameters of the bucket (with _finish_sh in the split step)
            self._bucket_clean = self.opt_deform is None and bool(getattr(self.opt_surfels, "zero_grads", False))
            if lanes:
                self.opt_surfels.grad2 = None

    def _update_torch(self, feature_idle):
        """CPU path: the two torch.optim.Adam (surfels | deformation), their schedules set on the host."""
        s = self.surfels
        if feature_idle:   # torch Adam skips parameters without a gradient, like the reference's detached deformation
            s.feature.grad = None
        if self.lr_schedule:
            k = self._steps_done
            for g in self.opt_surfels.param_groups:
                if g["name"] == "xyz":
                    g["lr"] = expon_lr(k, self.SCHED_POSITION[0], self.SCHED_POSITION[1], self.SCHED_POSITION[2]) * self._spatial
            self.opt_deform.param_groups[0]["lr"] = expon_lr(k, *self.SCHED_DEFORM)
        self._steps_done += 1
        self.opt_surfels.step()
        if not self.warmup:
            self.opt_deform.step()
        elif s.feature.grad is None:   # the flat bucket's view comes back for the next step
            s.feature.grad = self.bucket.flat[sum(p.numel() for p in self.bucket.params[:self.n_surfel_params - 1]):][:s.feature.numel()].view_as(s.feature)

    def _update_flat(self, n_train, adv, late, sh_done, mid_done, lanes, join):
        """HIP path: the flat Adam kernel over the parameter ranges that are still to do, next to whatever backward is still running.
        n_train: None, or (warm-up) the number of leading parameters that train; adv: this launch also runs the step guard;
        late: statistics of the view that were held back to go behind the surfel update (_fwd_bwd)."""
        s, opt, n_surf = self.surfels, self.opt_surfels, self.n_surfel_params
        if sh_done:
            first = n_surf if mid_done else 1
            if n_train is None or first < n_train:
                opt.step(first, n_train, advance=False)
        elif self.warmup:
            opt.step(0, n_surf if n_train is None else n_train, advance=adv)   # (never the deformation's parameters)
            if join is not None:
                torch.cuda.current_stream(s.get_xyz.device).wait_stream(join)
                self._accumulate_stats(lanes)
        elif join is not None:
            # concurrent lanes, single GPU: the surfels while the last lane's node-MLP backward runs on `join`; then everything else
            opt.step(0, n_surf, advance=adv)
            torch.cuda.current_stream(s.get_xyz.device).wait_stream(join)
            self._accumulate_stats(lanes)
            opt.step(n_surf, None, advance=False)
        elif getattr(self.deform, "_join_pending", False):
            # the node-MLP backward is still running on the side stream: update the surfels, which do
            # not depend on it, meanwhile; then join and update the deformation parameters
            opt.step(0, n_surf, advance=adv)
            if late is not None:
                self._statistics(*late)
                self._accumulate_stats(lanes)
            self.deform.join_backward()
            opt.step(n_surf, None, advance=False)
        else:
            opt.step(advance=adv)

    def view_for(self, iteration, j=0):
        """Shared deterministic schedule: step i renders views {(i k + j) world + rank} mod V, j = 0 .. k - 1 (k = views_per_rank)."""
        return self._scheduled_view(iteration, j)

    def _scheduled_view(self, iteration, j=0):
        """view_for's default order -- the one the captured step's device-side selection follows, whatever a caller put in view_for's place"""
        return ((iteration * self.views_per_rank + j) * self.world + self.rank) % len(self.cameras)

    # ---- k views per rank and step (opt-in lever of the data-parallel step) -------------------------------
    def _stats_accumulate(self, j):
        """The densification statistics of the step's j-th view into side buffers: the kernels of _statistics OVERWRITE the bucket
        tail and the radii; a multi-view step needs the SUM of the gradient norms and visibility counts and the MAX of the radii
        (add_densification_stats once per view, gaussian_model.py:484-486)."""
        if self._kx is None or self._kx.shape != self.bucket.extra.shape:
            self._kx = torch.zeros_like(self.bucket.extra)
            self._kr = torch.zeros_like(self._radii)
        if j == 0:
            self._kx.copy_(self.bucket.extra)
            self._kr.copy_(self._radii)
        else:
            self._kx.add_(self.bucket.extra)
            torch.maximum(self._kr, self._radii, out=self._kr)   # (element P, the overflow flag, is sticky: MAX keeps it)
        if j == self.views_per_rank - 1:
            self.bucket.extra.copy_(self._kx)
            self._radii.copy_(self._kr)

    def _loss_accumulate(self, j, loss):
        if self._kloss is None:
            self._kloss = torch.zeros(1, dtype=loss.dtype, device=loss.device)
        if j == 0:
            self._kloss.copy_(loss.reshape(1))
        else:
            self._kloss.add_(loss.reshape(1))
        if j == self.views_per_rank - 1:
            self._kloss.mul_(1.0 / self.views_per_rank)
            self._note_loss(self._kloss)

    def _view_of_step(self, j, cam, gt):
        """Forward + backward of the step's j-th view (views 1 .. k - 1 add to the gradients of view 0) and its statistics."""
        self._accum_view = j
        try:
            loss = self._fwd_bwd(cam, gt)
        finally:
            self._accum_view = 0
            if hasattr(self.deform, "reuse_knn"):
                # (stored neighbours are for views 2 .. k of THIS step only: a render from outside -- evaluation, a hook, after an in-place
                # densification that keeps the slot count -- must search again)
                self.deform.reuse_knn = False
        with torch.no_grad():
            self._stats_accumulate(j)
            self._loss_accumulate(j, loss)
        return loss

    def _multi_view_step(self, views):
        """One step over k views of this rank: gradients added view by view, then ONE exchange and ONE update -- the neighbour search,
        every all-reduce and the Adam kernels once per k views.  Not split (the SH all-reduce of the split step hides under ONE view's
        remaining backward; here k - 1 whole views run after the first one's gradients exist, and the exchange waits for the last)."""
        for j, v in enumerate(views):
            self._view_of_step(j, self.cameras[v], self.targets[v % len(self.targets)])
        self._finish()
        return self._kloss[0].detach().clone() if not self._graph else self._kloss

    def step(self):
        guarded = self.opt_deform is None and self._oflag is not None
        if guarded:
            self._check_guard()
            if not self._graph:   # eager launches read the context's current flag (a captured step has its own baked in)
                from diff_surfel_rasterization import _C
                _C.set_overflow_flag(self._oflag)
        if self.views_per_rank > 1:
            views = [self.view_for(self.iteration, j) for j in range(self.views_per_rank)]
            self.iteration += 1
            loss = self._step_views(views)
        else:
            v = self.view_for(self.iteration)
            self.iteration += 1
            loss = self._step_view(v)
        if guarded:
            self._guard_steps += 1
            ev = torch.cuda.Event()
            ev.record()
            self._guard_events[self._guard_steps] = ev
            if len(self._guard_events) > 2 * self.GUARD_RING:
                self._guard_events.pop(min(self._guard_events))
        return loss

    def _step_views(self, views):
        """A multi-view step (views_per_rank > 1): replay the captured per-view graphs, or run eagerly."""
        if self._graph:
            return self._replay_views(views)
        with trace.stage("dgs.step(%d views)" % len(views)):
            return self._multi_view_step_concurrent(views) if self._concurrent() else self._multi_view_step(views)

    def _step_view(self, v):
        if self._graph:
            return self._replay_view(v)
        cam, gt = self.cameras[v], self.targets[v % len(self.targets)]
        if self._split_ok():
            with trace.stage("dgs.step(split)"):
                return self._split_step(cam, gt)
        with trace.stage("dgs.forward+backward"):
            loss = self._fwd_bwd(cam, gt)
        with trace.stage("dgs.update"):
            self._finish()
        return loss
