"""The step guard of the captured step: a capacity overflow must not train anything, and the trainer recovers from it.

Mixin of dgs_amd.train.Trainer (its state: the optimiser, the bucket, the capture's capacity and list-length promise)."""
import torch
import torch.distributed as dist


class GuardMixin:
    # ---- step guard: a capacity overflow must not train anything -----------------------------------------------------
    #   _oflag: device overflow flag (one per trainer, shared with its lanes); None: no guarded step (torch.optim.Adam path)
    #   _radii: radii of the rendered view + 4 control ints ([P] = the flag's copy under data parallelism)
    #   _radii_scratch: split step -- where the statistics kernel writes the radii it does not own
    _oflag = _radii = _radii_scratch = None
    _in_recovery = False     # inside _recover_overflow's re-capture
    _capacity = 0            # list entries of the capture's capacity mode; 0: not captured yet
    _list_hint = None        # promised longest tile list (LIST_HINT_TIERS); None: not chosen yet (enable_graph starts at the first tier)
    GUARD_LAG = 2     # the host looks at the report of the step issued two steps earlier (already finished: no stall)
    GUARD_RING = 256  # entries of the pinned report ring (step, skipped flag, skipped so far, loss): also the loss history

    def _init_guard(self, old_opt=None):
        """Capacity mode has no host read inside the step, so a view whose tile lists do not fit renders as background and
        only raises a device flag (self._oflag, handed to the rasterizer).  The Adam and statistics kernels read that flag ON
        THE DEVICE and change nothing when it is set.  Data parallel: the flag rides as element P of the radii tensor through
        the step's MAX all-reduce (any rank's overflow stops every rank; no extra collective) and the kernels read the reduced
        copy.  The guard kernel also reports (step, flag, skipped) into a pinned ring that step() polls GUARD_LAG steps
        later -- the same lag on every rank, so all ranks recover at the same step: double the capacity, re-capture, and
        redo the skipped views."""
        dev = self.bucket.flat.device
        if self._oflag is None:
            self._oflag = torch.zeros(1, dtype=torch.int32, device=dev)
            self._ring = torch.zeros(self.GUARD_RING, 4, dtype=torch.float32).pin_memory()
        # radii of the rendered view (max over the ranks after the all-reduce) + 4 control ints; [P] = overflow flag
        self._radii = torch.zeros(self.P + 4, dtype=torch.int32, device=dev)
        self._radii_scratch = None
        opt = self.opt_surfels
        opt.skip = self._radii[self.P:self.P + 1] if self.world_size_hint() > 1 else self._oflag
        opt.host_ring = self._ring
        if old_opt is not None and hasattr(old_opt, "status"):   # rebuilt state (grow / node densification): counters carry over
            opt.status.copy_(old_opt.status)

    def world_size_hint(self):
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    def loss_history(self, k):
        """Losses of the last k steps (oldest first) from the guard kernel's pinned ring -- no copy kernel per step, no
        synchronisation inside the loop; synchronises here.  Steps that were skipped (capacity overflow) report their loss too."""
        assert 0 < k <= min(self.GUARD_RING, self._guard_steps), "only the last GUARD_RING steps are kept"
        torch.cuda.synchronize()
        out = []
        for n in range(self._guard_steps - k + 1, self._guard_steps + 1):
            e = self._ring[n % self.GUARD_RING]
            assert int(e[0]) == n, "ring entry overwritten"
            out.append(float(e[3]))
        return out

    def _check_guard(self):
        """Poll the report of the guarded step issued GUARD_LAG steps ago; recover if it (or, the flag being sticky, any
        step since) was skipped."""
        k = self._guard_steps - self.GUARD_LAG
        ev = self._guard_events.pop(k, None)
        if k < 1 or ev is None:
            return
        ev.synchronize()
        e = self._ring[k % self.GUARD_RING]
        if int(e[0]) != k:
            # the device's step counter and the host's disagree (something advanced FlatAdam outside step()): resynchronise
            # and look at the flag itself -- silently ignoring the report would hide an overflow for good
            self._resync_guard()
            # (data parallel: only what EVERY rank sees may decide -- the guard kernel's copy of the MAX-reduced flag, not this rank's own)
            if float(self.opt_surfels.status[0].item()) > 0 or (self.world == 1 and bool(self._oflag.item())):
                self._recover_overflow()
            return
        if float(e[1]) > 0:
            self._recover_overflow()

    def _flush_guard(self):
        """Look at every report the step guard has not shown the host yet (step() polls GUARD_LAG steps late) and recover if one of
        them -- or the sticky flag itself -- says a step was skipped.  Called wherever the trainer is about to re-capture, change
        the slot layout or save: an overflow of the last two steps must not be captured into a fresh graph as a stale flag, withdraw
        the list-length promise for good, or be lost with the steps it skipped."""
        self._wait_gather()
        if self.opt_deform is not None or self._oflag is None or self._in_recovery:
            return False
        torch.cuda.synchronize()
        self._guard_events.clear()
        skipped = int(self.opt_surfels.status[1].item())
        # data parallel: the skipped-step count comes from the MAX-reduced flag and is the same on every rank; this rank's own flag is
        # not (a recovery is collective: every rank must take this branch, or none)
        if skipped != self._skipped_seen or (self.world == 1 and bool(self._oflag.item())):
            if self._graph and self._capacity > 0:
                self._recover_overflow()
                return True
            raise RuntimeError("rasterizer capacity overflow outside capacity mode")
        return False

    def _recover_overflow(self):
        torch.cuda.synchronize()
        skipped = int(self.opt_surfels.status[1].item())
        redo = skipped - self._skipped_seen
        self._skipped_seen = skipped
        if not self._graph or self._capacity <= 0:
            raise RuntimeError("rasterizer capacity overflow outside capacity mode")
        self.iteration -= redo          # the skipped steps changed nothing: their views are rendered again
        # binning_kernels.h overflow_reason: 1 capacity, 2 promised list length, 4 beyond the segmented sort -- the bits of EVERY rank's
        # flag (the step's MAX all-reduce only says that some rank overflowed, and max(1, 2) drops a bit): all ranks must move to the
        # same capacity and the same promise, or their captures -- and the collectives inside the capture's warm-up steps -- diverge
        reason = self._agree_reason(int(self._oflag.item()))
        self._oflag.zero_()
        self._guard_events.clear()
        self.overflow_recoveries += 1
        self._after_overflow(reason)
        self._graph = None
        self._in_recovery = True
        try:
            self.enable_graph(self._capacity, validate=False)
        finally:
            self._in_recovery = False

    def _agree_reason(self, reason):
        """Overflow reason bits OR-ed over the ranks (collective: every rank calls it at the same point).  The bits travel as three
        0/1 words through a MAX all-reduce -- RCCL has no bitwise OR reduction."""
        if self.world > 1 and not self.no_collectives and dist.is_initialized():
            bits = torch.tensor([reason & 1, (reason >> 1) & 1, (reason >> 2) & 1], dtype=torch.int32, device=self.bucket.flat.device)
            dist.all_reduce(bits, op=dist.ReduceOp.MAX)
            b = bits.tolist()
            reason = (reason & ~7) | b[0] | (b[1] << 1) | (b[2] << 2)
        return reason

    # Promise of the longest tile list (dgs_set_option key 6) in the tiers of the library's sort kernels: up to 2048 entries one
    # launch, up to 57 344 (28 segments of 2048 + merge) three, no promise (0) four.  A view that breaks the promise
    # moves the trainer one tier up -- a densified scene with lists of a few thousand entries keeps the cheap tiers it fits.
    LIST_HINT_TIERS = (2048, 57344, 0)

    def _after_overflow(self, reason):
        """The next configuration after a frame that did not fit, from the reason bits the kernels left in the flag: a broken promise
        moves the list-length tier (straight to 'no promise' when the list is beyond the segmented sort), a full buffer doubles the
        capacity -- both in ONE recovery when both happened.  reason == 0 (flag already consumed): the order of rounds 3-4, promise first."""
        hint = self._list_hint or 0
        if reason & 6 and hint:
            self._list_hint = 0 if reason & 4 else self._next_list_hint()
        if reason & 1:
            self._capacity = 2 * self._capacity
        if not reason & 7:
            if hint:
                self._list_hint = self._next_list_hint()
            else:
                self._capacity = 2 * self._capacity

    def _next_list_hint(self):
        t = self.LIST_HINT_TIERS
        cur = self._list_hint or 0
        return t[t.index(cur) + 1] if cur in t and cur != 0 else 0

    def _resync_guard(self):
        """The guard kernel numbers its reports with the DEVICE step counter (status[2]); whoever moves that counter behind the
        trainer's back -- a restored snapshot, a tool that drives FlatAdam.step directly -- must bring the host's copy along, or
        no report would ever match its ring slot again (and a sticky overflow would freeze training unnoticed)."""
        if self.opt_deform is None and hasattr(self.opt_surfels, "status"):
            torch.cuda.synchronize()
            self._guard_steps = int(self.opt_surfels.status[2].item())
            self._guard_events.clear()
