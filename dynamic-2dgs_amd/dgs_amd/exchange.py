"""The data-parallel exchange of a step: the asynchronous slices of the gradient bucket (all-reduce, sharded SH update, bf16 wire),
the updates that follow each slice, and the ONE order in which the split step starts and waits for them (_split_exchange).

Mixin of dgs_amd.train.Trainer."""
import torch
import torch.distributed as dist


class ExchangeMixin:
    _wire = None    # persistent bfloat16 staging copy of the bucket (wire_bf16), built by _wire_slice

    def _n_mid(self):
        """Elements of the second bucket segment: the surfel parameters behind the SH coefficients."""
        return sum(p.numel() for p in self.bucket.params[1:self.n_surfel_params])

    class _NoWork:
        """stand-in for the work handle of a collective that was not issued (Trainer.no_collectives)"""
        @staticmethod
        def wait():
            return True

    class _Bf16Work:
        """work handle of a slice that crossed the wire as bfloat16: wait() = the collective, then the copy back into the fp32 bucket"""
        def __init__(self, work, dst, src):
            self.work, self.dst, self.src = work, dst, src

        def wait(self):
            self.work.wait()
            self.dst.copy_(self.src)
            return True

    def _wire_slice(self, lo, hi):
        """bucket.flat[lo:hi] copied into the persistent bfloat16 staging buffer (as long as the bucket; rebuilt when the bucket was):
        the view of it that crosses the wire instead of the fp32 slice"""
        flat = self.bucket.flat
        if self._wire is None or self._wire.numel() != flat.numel() or self._wire.device != flat.device:
            self._wire = torch.empty(flat.numel(), dtype=torch.bfloat16, device=flat.device)
        w = self._wire[lo:hi]
        w.copy_(flat[lo:hi])
        return w

    def _sum_slice_start(self, lo, hi):
        """async all-reduce (SUM) of bucket.flat[lo:hi]; with wire_bf16 through a persistent bfloat16 copy of the slice"""
        sl = self.bucket.flat[lo:hi]
        if not self.wire_bf16:
            return dist.all_reduce(sl, op=dist.ReduceOp.SUM, async_op=True)
        w = self._wire_slice(lo, hi)
        return self._Bf16Work(dist.all_reduce(w, op=dist.ReduceOp.SUM, async_op=True), sl, w)

    # ---- sharded SH update (data parallel, split step) ------------------------------------------------------------------
    def _shard_ok(self):
        """Does the split step hand the SH update to the rows' owners (Trainer.shard_optimizer)?  Needs equal row ranges."""
        if not (self.shard_optimizer and dist.is_available() and dist.is_initialized() and self._split_ok()):
            return False
        return self.P % dist.get_world_size() == 0 and self.n_sh % self.P == 0

    def _shard_range(self):
        """ELEMENT range of the SH segment (bucket and parameter alike) this rank owns: rows [rank P / N, (rank + 1) P / N)."""
        n, r = dist.get_world_size(), dist.get_rank()
        c = self.n_sh // n
        return r * c, (r + 1) * c

    def _scatter_sh_start(self):
        """async reduce-scatter (SUM) of the SH gradients, in place: this rank's rows of the bucket receive the sum over the ranks
        (the other rows keep this rank's own contribution and are overwritten by the next backward).  With wire_bf16 through the
        persistent bfloat16 copy, like _sum_slice_start."""
        lo, hi = self._shard_range()
        sl = self.bucket.flat[:self.n_sh]
        if not self.wire_bf16:
            return dist.reduce_scatter_tensor(sl[lo:hi], sl, op=dist.ReduceOp.SUM, async_op=True)
        w = self._wire_slice(0, self.n_sh)
        return self._Bf16Work(dist.reduce_scatter_tensor(w[lo:hi], w, op=dist.ReduceOp.SUM, async_op=True), sl[lo:hi], w[lo:hi])

    def _gather_sh_start(self):
        """async all-gather of the SH rows every rank has just updated, IN PLACE into the parameter.  Nothing of this step reads the SH
        coefficients any more; the next reader is the next step's preprocess kernel, behind that step's deformation head
        (_wait_gather sits between the two) -- or whoever calls settle_shards()."""
        self._sh_moments_local = True
        if self.no_collectives:
            return
        f = self.surfels._features.data.view(-1)
        lo, hi = self._shard_range()
        self._ag_work = dist.all_gather_into_tensor(f, f[lo:hi], async_op=True)

    def _wait_gather(self):
        """The current stream waits for the outstanding all-gather of the SH coefficients (if any)."""
        if self._ag_work is not None:
            self._ag_work.wait()
            self._ag_work = None

    def settle_shards(self):
        """Make this rank's copy of everything complete again: wait for the SH all-gather and, if the SH moments are only current
        on their owners' rows, all-gather them too (two collectives: EVERY rank must call this at the same point -- it is called
        by whatever reads moments across rows or replaces the optimiser state: densification, reordering, growth, checkpoints)."""
        self._wait_gather()
        if self._sh_moments_local and self.opt_deform is None and dist.is_available() and dist.is_initialized() and not self.no_collectives:
            lo, hi = self._shard_range()
            a = self.opt_surfels._offsets[0]
            for m in (self.opt_surfels.exp_avg, self.opt_surfels.exp_avg_sq):
                seg = m[a:a + self.n_sh]
                dist.all_gather_into_tensor(seg, seg[lo:hi])
        self._sh_moments_local = False

    def _reduce_mid_start(self):
        if self.no_collectives:
            return self._NoWork
        return self._sum_slice_start(self.n_sh, self.n_sh + self._n_mid())

    def _finish_mid(self):
        """Third split: the surfel parameters behind the SH coefficients, as soon as THEIR all-reduce is in."""
        with torch.no_grad():
            self.opt_surfels.grad_scale = 1.0 / self.world
            self.opt_surfels.step(1, self.n_surfel_params - 1 if self.warmup else self.n_surfel_params, advance=False)

    def _reduce_sh_start(self):
        if self.no_collectives:
            return self._NoWork
        if self._shard_ok():
            return self._scatter_sh_start()
        return self._sum_slice_start(0, self.n_sh)

    def _reduce_radii_start(self):
        if self.no_collectives:
            return self._NoWork
        return dist.all_reduce(self._radii, op=dist.ReduceOp.MAX, async_op=True)

    def _reduce_rest_start(self, mid_left=False):
        """async all-reduce of what is behind the SH segment -- mid_left: and behind the per-surfel segment, which left earlier"""
        if self.no_collectives:
            return []
        return [dist.all_reduce(self.bucket.flat[self.n_sh + (self._n_mid() if mid_left else 0):], op=dist.ReduceOp.SUM, async_op=True)]

    def wire_bytes_per_step(self):
        """Bytes each rank hands to the collectives per step (payload of the all-reduces; what actually crosses the links is
        2 (n-1)/n times that for a ring).  {'sh': SH gradients (all-reduced while the rest of the backward runs), 'rest': all
        other gradients + the densification statistics of the view, 'radii': int32 radii + the overflow flag (MAX)}."""
        n_flat = self.bucket.flat.numel()
        n_radii = self.P + 4
        sh = self.n_sh if self._split_ok() else 0
        big = 2 if (self.wire_bf16 and sh) else 4   # bytes per element of the slices that can cross as bfloat16
        out = {"sh": big * sh, "rest": 4 * (n_flat - sh), "radii": 4 * n_radii}
        if sh and self.split3:   # 'mid' leaves when the skinning backward is done, 'rest' (deformation parameters + statistics) last
            out["mid"] = big * self._n_mid()
            out["rest"] -= 4 * self._n_mid()
        out["total"] = sum(out.values())
        return out

    @property
    def _fold_mean(self):
        """Flat Adam kernel: the bucket keeps the SUM over the ranks and the kernel reads grad / world (no averaging pass)."""
        return self.opt_deform is None and self.world > 1

    def _reduce(self):
        if self.no_collectives:
            return
        self.bucket.all_reduce_mean(average=not self._fold_mean)
        if self.world > 1:
            dist.all_reduce(self._radii, op=dist.ReduceOp.MAX)

    def _finish_sh(self):
        """Data-parallel split step: the SH coefficients (first bucket segment, first parameter) can be updated as soon as their
        all-reduce is done -- while the rest of the bucket is still on the wire."""
        with torch.no_grad():
            self.opt_surfels.grad_scale = 1.0 / self.world
            if self._shard_ok():   # this rank's rows only (their gradient sum arrived by reduce-scatter); _gather_sh_start follows
                self.opt_surfels.step_slice(0, *self._shard_range())
            else:
                self.opt_surfels.step(0, 1)

    def _split_exchange(self, head, half_a, half_b, half_b2, finish_sh, finish_mid, finish_rest):
        """The data-parallel split step: backward half a | SH reduce (async) | backward half b | reduce of the rest (async) | SH
        update | update of everything else.  THE order of collective starts and waits -- it must be the same on every rank and in
        the eager and the captured step, so both run it from here and hand in their stages: bound methods (_split_step) or the
        captured graphs' replay (_replay_view).
        head: the deformation head as a stage of its own (sharded SH update: it reads no SH coefficient, so the wait for the
        all-gather of the previous step's SH rows sits BEHIND it and that transfer rides under the head's ~75 us), or None; what it
        returns goes to half_a.  half_b2 / finish_mid: the third split (per-surfel gradients leave under the node-MLP backward),
        or None.  Returns what half_a returned."""
        h = None
        if head is not None:
            h = head()
            self._wait_gather()
        loss = half_a(h)
        rwork = self._reduce_radii_start()   # radii + overflow flag (small): first, the SH update's guard reads it
        work = self._reduce_sh_start()       # runs on the collective's stream while half b runs
        half_b()
        mid = None
        if half_b2 is not None:
            mid = self._reduce_mid_start()
            half_b2()
        rest = self._reduce_rest_start(mid_left=mid is not None)
        rwork.wait()
        work.wait()
        finish_sh()                          # SH update while the rest of the bucket is on the wire
        if head is not None:
            self._gather_sh_start()          # ... and its rows go out behind the rest, under the other updates and the next head
        if mid is not None:
            mid.wait()
            finish_mid()
        for w in rest:
            w.wait()
        finish_rest()
        return loss

    def _split_step(self, cam, gt):
        """Data-parallel step, eager: _split_exchange over the bound methods."""
        third = self.split3
        return self._split_exchange(
            (lambda: self._forward_head(cam)) if self._shard_ok() else None, lambda head: self._fwd_bwd_a(cam, gt, head),
            self._fwd_bwd_b1 if third else self._fwd_bwd_b, self._fwd_bwd_b2 if third else None, self._finish_sh, self._finish_mid,
            lambda: self._finish(reduce=False, sh_done=True, mid_done=third))
