"""Parameter surgery of a running trainer: adaptive density control, the storage order of surfels and nodes, growth of the slot
count, node densification, holding parameters back over a step, adopting another optimiser's state -- everything that moves rows of
parameters together with their Adam moments and statistics.

Mixin of dgs_amd.train.Trainer."""
import torch


class SurgeryMixin:
    # ---- adaptive density control (train_gui.py:410-423; dgs_amd/densify.py) -----------------------------------------
    def _moments(self):
        from . import densify
        self.settle_shards()
        return self.opt_surfels.moments if self.opt_deform is None else densify.TorchAdamMoments(self.opt_surfels)

    def densify_and_prune(self, max_grad=0.0002, min_opacity=0.01, extent=1.0, max_screen_size=None, percent_dense=0.01,
                          noise=None, seed=0):
        """Clone / split / prune in place (no re-allocation, captured graphs stay valid).  Identical on every rank: the
        statistics were summed over the ranks by the step, the random draw is seeded by (seed, iteration).
        Returns (n_cloned, n_split, n_pruned)."""
        from . import densify
        self._flush_guard()   # the statistics of a skipped step must be redone before they are used
        dev = self.surfels.get_xyz.device
        gen = torch.Generator(device=dev).manual_seed(int(seed) * 1000003 + self.iteration)
        args = (max_grad, min_opacity, extent, max_screen_size)
        out = densify.densify_and_prune(self.surfels, self._moments(), *args, percent_dense=percent_dense, noise=noise, generator=gen)
        if isinstance(out, int):   # slots exhausted: the one case that re-allocates (and re-captures)
            # a dead slot still costs the per-surfel kernels their share of the step: grow by a quarter, not by multiples
            self.grow(-(-max(int(1.25 * self.P), self.P + 2 * out) // 1024) * 1024)
            out = densify.densify_and_prune(self.surfels, self._moments(), *args, percent_dense=percent_dense, noise=noise, generator=gen)
        return out

    def reset_opacity(self):
        from . import densify
        self._flush_guard()
        densify.reset_opacity(self.surfels, self._moments())

    # ---- storage order of the surfels ------------------------------------------------------------------------------------
    @torch.no_grad()
    def reorder_surfels(self, perm):
        """Permute the surfel slots IN PLACE (new slot i <- old slot perm[i]): parameters, both Adam moments, densification
        statistics, the alive mask, the neighbour-search seed.  No address changes, so captured graphs stay valid.  The order
        of the surfels carries no meaning (the reference appends and deletes rows freely); outputs change only through
        ties between equal-depth surfels (broken by index) and floating-point summation order."""
        from . import densify
        s = self.surfels
        perm = perm.to(s.get_xyz.device)
        assert perm.shape == (self.P,)
        moments = self._moments()
        for p in densify.surfel_rows(s).values():
            p.data.copy_(p.data[perm])
            for m in moments(p):
                if m is not None:
                    m.copy_(m[perm])
        for name in ("xyz_gradient_accum", "denom", "max_radii2D", "alive"):
            b = getattr(s, name)
            b.copy_(b[perm])
        seed = getattr(self.deform, "_knn_seed", None)
        if seed is not None and seed.shape[0] == self.P:
            seed.copy_(seed[perm])

    @torch.no_grad()
    def reorder_nodes(self, perm):
        """Permute the control nodes IN PLACE (new row i <- old row perm[i]): positions + hyper coordinates, radius, weight,
        their Adam moments; the node indices held in the neighbour-search seed are renamed.  The order of the nodes carries
        no meaning (the MLP is evaluated per node, skinning sums over a surfel's K neighbours)."""
        d = self.deform
        perm = perm.to(d.nodes.device)
        M = d.nodes.shape[0]
        assert perm.shape == (M,)
        for p in (d.nodes, d._node_radius, d._node_weight):
            p.data.copy_(p.data[perm])
            for m in self._any_moments(p):
                if m is not None:
                    m.copy_(m[perm])
        seed = getattr(d, "_knn_seed", None)
        if seed is not None:
            new_of_old = torch.empty_like(perm)
            new_of_old[perm] = torch.arange(M, device=perm.device)
            ok = (seed >= 0) & (seed < M)
            seed.copy_(torch.where(ok, new_of_old[seed.clamp(0, M - 1)], seed))

    @torch.no_grad()
    def sort_nodes(self):
        """Store the control nodes along a Morton curve through their bounding box (padding nodes last): 32 consecutive nodes
        then fill a small box, which is what lets dgs_knn_refine skip most 32-node blocks for a wave of neighbouring surfels."""
        d = self.deform
        x = d.nodes.detach()[:, :3]
        live = d.live_nodes if hasattr(d, "live_nodes") else torch.ones(x.shape[0], dtype=torch.bool, device=x.device)
        if callable(live):
            live = live()
        if not bool(live.any()):
            return
        lo, hi = x[live].min(0).values, x[live].max(0).values
        q = ((x - lo) / (hi - lo).clamp_min(1e-12) * 1023.0).clamp(0, 1023).to(torch.int64)
        code = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
        for b in range(10):
            for c in range(3):
                code |= ((q[:, c] >> b) & 1) << (3 * b + c)
        code = torch.where(live, code, torch.full_like(code, 1 << 40))
        self.reorder_nodes(torch.argsort(code, stable=True))

    @torch.no_grad()
    def sort_surfels(self):
        """Store the surfels in the order of their nearest control node (dead slots last).  On MI355X this is what makes the
        per-surfel kernels of the deformation coherent: the 64 surfels of a wave then read the same one or two node rows
        (broadcast loads), and the skinning backward can sum a wave's contributions to a node in registers and issue one
        atomic per (wave, node) (dgs_deform_backward, coherent variant; 97 -> ~20 us at 200 k surfels / 1024 nodes) instead
        of building 256 LDS tables.  Call after initialisation and after densification; stale order only costs time."""
        self._flush_guard()
        s, d = self.surfels, self.deform
        self.sort_nodes()
        x, nodes = s.get_xyz.detach(), d.nodes.detach()[:, :3]
        near = torch.cat([torch.cdist(x[i:i + 16384], nodes).argmin(1) for i in range(0, x.shape[0], 16384)])
        near = torch.where(s.alive, near, torch.full_like(near, nodes.shape[0]))
        self.reorder_surfels(torch.argsort(near, stable=True))
        d.coherent_surfels = bool(x.is_cuda and self.rasterizer_cls is None)

    def grow(self, capacity):
        """Re-allocate the surfel slots (parameters, gradient bucket, Adam moments, statistics) to `capacity` and re-capture
        the step's graphs if they were enabled.  Values, moments and the Adam step count carry over."""
        from . import densify
        self._flush_guard()
        s = self.surfels
        old = s.get_xyz.shape[0]
        assert capacity > old
        moments = self._moments()
        rows = densify.surfel_rows(s)
        saved = {name: tuple(None if t is None else t.detach().clone() for t in moments(p)) for name, p in rows.items()}
        deform_saved = [tuple(None if t is None else t.detach().clone() for t in self._param_moments(p)) for p in self.deform.parameters()]
        if self.opt_deform is None:
            t_saved = self.opt_surfels.t.clone()
        else:
            t_saved = {name: self.opt_surfels.state[p].get("step") for name, p in rows.items() if p in self.opt_surfels.state}
        fill = {"opacity": densify.DEAD_LOGIT, "scaling": -6.0, "feature": -1e-2}
        attr = {"xyz": "_xyz", "f_all": "_features", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
                "scaling": "_scaling", "rotation": "_rotation", "feature": "feature"}
        n = capacity - old
        with torch.no_grad():
            for name, p in rows.items():
                pad = torch.full((n,) + tuple(p.shape[1:]), fill.get(name, 0.0), dtype=p.dtype, device=p.device)
                if name == "rotation":
                    pad[:, 0] = 1
                setattr(s, attr[name], torch.nn.Parameter(torch.cat((p.detach(), pad)).contiguous()))
            for name in ("xyz_gradient_accum", "denom", "max_radii2D", "alive"):
                b = getattr(s, name)
                setattr(s, name, torch.cat((b, torch.zeros((n,) + tuple(b.shape[1:]), dtype=b.dtype, device=b.device))))
        self._half = None
        self._radii = None
        self._build_state()
        moments = self._moments()
        with torch.no_grad():
            if self.opt_deform is None:
                self.opt_surfels.t.copy_(t_saved)
            for name, p in densify.surfel_rows(s).items():
                m0, v0 = saved[name]
                if m0 is None:
                    continue
                if self.opt_deform is not None:   # torch Adam creates its state lazily
                    self.opt_surfels.state[p] = {"step": t_saved[name], "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                m, v = moments(p)
                m[:old] = m0
                v[:old] = v0
            for p, (m0, v0) in zip(self.deform.parameters(), deform_saved):
                if m0 is not None and self.opt_deform is None:
                    m, v = self.opt_surfels.moments(p)
                    m.copy_(m0)
                    v.copy_(v0)
        if self._graph:
            # the list capacity follows the slot count (the same entries per surfel as before)
            self._capacity = int(-(-self._capacity * capacity // old))
            self._recapture()

    def densify_nodes(self, max_grad=0.0002):
        """DeformModel.densify (train_gui.py:413-415, utils/time_utils.py:1286-1385) with the surfels' accumulated view-space
        gradient.  The node count changes, so the bucket / optimiser are rebuilt (moments and step count carry over) and the
        step is re-captured; on the HIP path the count is padded to a multiple of 64 (fused MLP kernels) with unreachable
        nodes.  Returns (n_added, n_pruned) or None if nothing changed."""
        self._flush_guard()
        s, d = self.surfels, self.deform
        fused = self.opt_deform is None
        with torch.no_grad():
            x_grad = s.xyz_gradient_accum / s.denom
            alive = s.alive
            old = {id(p): tuple(None if t is None else t.detach().clone() for t in self._any_moments(p)) for p in self.bucket.params}
            t_saved = self.opt_surfels.t.clone() if fused else None
            # torch Adam counts steps per parameter (a parameter's count starts with its first gradient: the deformation's after the
            # warm-up); the reference's surgery keeps each state's count, and the re-sized node tensors inherit their predecessors'
            steps = {}
            if not fused:
                for opt in (self.opt_surfels, self.opt_deform):
                    steps.update({id(p): st["step"].clone() for p, st in opt.state.items() if "step" in st})
                node_steps = {n: steps.get(id(getattr(d, n))) for n in ("nodes", "_node_radius", "_node_weight")}
            res = d.densify_nodes(max_grad, s.get_xyz.detach()[alive], x_grad[alive], s.feature.detach()[alive], moments=self._any_moments,
                                  pad_to=64 if fused else 1)
            if res is None:
                return None
            n_add, n_prune, node_moments = res
            if not fused:   # torch Adam keyed its state by the replaced parameter objects
                self.opt_deform = None
            self._half = None
            self._build_state()
            new_nodes = {id(getattr(d, n)): mv for n, mv in node_moments.items()}
            if not fused:
                steps.update({id(getattr(d, n)): t for n, t in node_steps.items() if t is not None})
            if fused:
                self.opt_surfels.t.copy_(t_saved)
            for p in self.bucket.params:
                m0, v0 = new_nodes.get(id(p), old.get(id(p), (None, None)))
                if m0 is None:
                    continue
                if not fused:
                    opt = self.opt_deform if any(p is q for g in self.opt_deform.param_groups for q in g["params"]) else self.opt_surfels
                    opt.state[p] = {"step": steps.get(id(p), torch.tensor(float(self._steps_done))).clone(), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
                else:
                    m, v = self.opt_surfels.moments(p)
                    m.copy_(m0)
                    v.copy_(v0)
        self._recapture()
        return n_add, n_prune

    def _any_moments(self, p):
        """Adam moments of any parameter of the bucket, whichever optimiser holds it."""
        if self.opt_deform is None:
            return self.opt_surfels.moments(p)
        for opt in (self.opt_surfels, self.opt_deform):
            st = opt.state.get(p, None)
            if st:
                return st["exp_avg"], st["exp_avg_sq"]
        return None, None

    def _param_moments(self, p):
        if self.opt_deform is None:
            return self.opt_surfels.moments(p)
        return (None, None)

    @torch.no_grad()
    def hold_surfels(self, nodes=False):
        """Copies of the per-surfel parameters (nodes=True: of the three node tensors instead) and of their Adam state;
        release_surfels puts them back.  Around a step: the step trains everything else and gathers the densification statistics, the
        held parameters stay where they were -- what the reference does to parameters its density control replaces in front of the
        optimiser's step (dgs_amd.fit.run_iteration)."""
        from . import densify
        self.settle_shards()
        d = self.deform
        params = [d.nodes, d._node_radius, d._node_weight] if nodes else list(densify.surfel_rows(self.surfels).values())
        held = []
        for p in params:
            m, v = self._any_moments(p)
            st = self._torch_state(p)
            held.append((p, p.detach().clone(), None if m is None else m.clone(), None if v is None else v.clone(),
                         None if not st else st["step"].clone()))
        return held

    def _torch_state(self, p, pop=False):
        """torch.optim.Adam's state entry of parameter p (CPU path; the optimisers may have been rebuilt since a hold), or None."""
        if self.opt_deform is None:
            return None
        for opt in (self.opt_surfels, self.opt_deform):
            if p in opt.state:
                return opt.state.pop(p) if pop else opt.state[p]
        return None

    @torch.no_grad()
    def release_surfels(self, held):
        self.settle_shards()
        for p, value, m0, v0, step in held:
            p.copy_(value)
            m, v = self._any_moments(p)
            if m0 is not None:
                m.copy_(m0)
                v.copy_(v0)
            elif m is not None:   # a parameter that saw its first update in this step (torch Adam): back to no state
                self._torch_state(p, pop=True)
            if step is not None:
                self._torch_state(p)["step"].copy_(step)

    @torch.no_grad()
    def adopt_deform_state(self, adam):
        """Continue a torch.optim.Adam's state for the deformation parameters: in the reference ONE optimiser of the deformation
        model runs through the node pre-training stage and the joint stage (scene/deform_model.py:26-33, train_gui.py:590-592 and
        :429-431), so the joint stage starts with the moments and the per-parameter step counts the first stage left.  `adam`: the
        optimiser of dgs_amd.node_pretrain.NodePretrainer (same Parameter objects).  Before enable_graph: the step origins are
        kernel arguments.  Returns the number of parameters whose state was taken over."""
        n = 0
        if self.opt_deform is not None:
            for p, st in adam.state.items():
                self.opt_deform.state[p] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                n += 1
            return n
        assert self._graph is None, "adopt_deform_state before enable_graph"
        flat = self.opt_surfels
        for i, p in enumerate(flat.params):
            st = adam.state.get(p)
            if not st:
                continue
            m, v = flat.moments(p)
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            flat.set_origin(i, i + 1, float(self._steps_done) - float(st["step"]))   # bias corrections continue at step + 1
            self._adopted_steps[i] = float(st["step"])   # (the end of the warm-up re-bases the origins: set_regime)
            n += 1
        return n
