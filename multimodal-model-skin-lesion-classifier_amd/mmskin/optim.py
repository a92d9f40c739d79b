"""Adam for models whose backbone keeps its parameters in ONE flat arena (mmskin/backbone.py): a drop-in for the
`torch.optim.Adam(model.parameters(), lr=..., weight_decay=...)` of the reference's training scripts
(/root/reference/src/scripts/benchmark/train_pad_20.py:54, stepped at :113).

Every run of parameters that are consecutive views of one fp32 CUDA storage, with gradients that are consecutive views of one
gradient storage at the same offsets (what the plan-executed backward hands out), is stepped by ONE launch of `mmskin_adam_step`
over the whole range -- moments live in two flat tensors, `state[p]['exp_avg']` / `['exp_avg_sq']` are views of them, so
`state_dict()` / `load_state_dict()` keep torch's layout.  Everything else (the head's parameters, CPU tensors, amsgrad /
maximize / capturable / tensor-lr groups) goes through torch.optim.Adam's own step.  Same update rule, same state keys.

The kernel takes ONE step count, so a run never holds members whose counts differ: a parameter that joins later (its gradient
was None, or it skipped a step) starts a run of its own and keeps its own bias correction, as in torch.  The counts are kept on
the host (`self._t`); a `state[p]['step']` tensor is read only when a parameter enters a run with state this optimizer did not
count itself (after `load_state_dict()` or a GradScaler step), never in a steady-state step.

Under `torch.amp.GradScaler` (`fused=True` makes it hand `grad_scale` / `found_inf` to `step()` instead of unscaling) the whole
step is torch's: its fused kernel divides by the scale and skips on an inf.  It updates the views of the flat moments in place,
so the runs stay as they are."""
import torch

from . import _lib
from ._lib import call, ptr, stream

_MIN_RUN = 1 << 16     # elements: shorter runs stay with torch's multi-tensor path


class Adam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
        self._runs = {}    # (group index, first parameter id, members) -> dict(params, n, m, v, step, cell, views): the LIVE runs only
        self._t = {}       # parameter -> cell [its state's step tensor, host copy of the count or None = not read yet]; a run's members share one cell
        self._loose = {}   # the parameters of _t that are in no run (torch steps them): their cells are counted up after torch's step

    def _count(self, q):
        """q's step count without a device read, unless its `step` tensor is one this optimizer has not counted itself."""
        s = self.state.get(q, {}).get("step")
        if s is None:
            return 0
        c = self._t.get(q)
        if c is None or c[0] is not s:
            c = self._t[q] = self._loose[q] = [s, None]
        if c[1] is None:
            c[1] = int(float(s))
        return c[1]

    # ---- consecutive runs of one group's parameters inside a shared storage, gradients laid out alike
    @staticmethod
    def _find_runs(params, count=None):
        """count(p) -> step count: neighbours whose counts differ are in different runs (None: the layout alone decides)."""
        by_store = {}
        for p in params:
            g = p.grad
            if (g is None or not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or g.is_sparse
                    or not p.is_contiguous() or not g.is_contiguous()):
                continue
            by_store.setdefault((p.untyped_storage().data_ptr(), g.untyped_storage().data_ptr()), []).append(p)
        runs = []
        for ps in by_store.values():
            if len(ps) < 2:
                continue
            ps.sort(key=lambda q: q.storage_offset())
            cur = [ps[0]]
            for q in ps[1:]:
                a = cur[-1]
                if (q.storage_offset() == a.storage_offset() + a.numel()
                        and q.grad.storage_offset() - q.storage_offset() == a.grad.storage_offset() - a.storage_offset()):
                    cur.append(q)
                else:
                    runs.append(cur); cur = [q]
            runs.append(cur)
        ok = lambda r: sum(q.numel() for q in r) >= _MIN_RUN and r[0].data_ptr() % 16 == 0 and r[0].grad.data_ptr() % 16 == 0
        if count is None:
            return [r for r in runs if ok(r)]
        out = []
        for r in runs:
            if sum(q.numel() for q in r) < _MIN_RUN:    # too short whatever the counts are: no count is looked at
                continue
            cur, t = [r[0]], count(r[0])
            for q in r[1:]:
                tq = count(q)
                if tq == t:
                    cur.append(q)
                else:
                    out.append(cur); cur, t = [q], tq
            out.append(cur)
        return [r for r in out if ok(r)]     # a piece may start off a 16-byte boundary, or be short: torch steps it

    def _bound(self, st):
        """every member's state is still this run's: a load_state_dict() replaces the per-parameter tensors"""
        return all(self.state.get(q, {}).get("exp_avg") is mv and self.state[q].get("step") is st["step"]
                   for q, (mv, _) in zip(st["params"], st["views"]))

    def _run_state(self, key, run):
        st = self._runs.get(key)
        if st is not None and len(st["params"]) == len(run) and all(a is b for a, b in zip(st["params"], run)) and self._bound(st):
            return st
        n = sum(q.numel() for q in run)
        dev = run[0].device
        fused = self.param_groups[key[0]].get("fused")
        t = self._count(run[0])      # _find_runs put equal counts together
        m = torch.zeros(n, dtype=torch.float32, device=dev)
        v = torch.zeros(n, dtype=torch.float32, device=dev)
        step_t = torch.full((), float(t), dtype=torch.float32, device=dev if fused else "cpu")   # where torch keeps it
        cell, off, views = [step_t, t], 0, []
        for q in run:
            k = q.numel()
            old = self.state.get(q, {})
            if "exp_avg" in old:     # per-parameter state (torch's own, a reload, or a view of another run's moments): fold it in
                m[off:off + k].copy_(old["exp_avg"].reshape(-1)); v[off:off + k].copy_(old["exp_avg_sq"].reshape(-1))
            mv, vv = m[off:off + k].view(q.shape), v[off:off + k].view(q.shape)
            self.state[q] = {"step": step_t, "exp_avg": mv, "exp_avg_sq": vv}
            self._t[q] = cell
            self._loose.pop(q, None)
            views.append((mv, vv))
            off += k
        if st is not None:
            self._drop(st)           # the entry this one replaces: whoever it still holds is on its own now
        st = dict(params=list(run), n=n, m=m, v=v, step=step_t, cell=cell, views=views)
        self._runs[key] = st
        return st

    def _drop(self, st):
        """A run that is no longer stepped as one: the members it still holds get a step tensor and moments of their own, so that
        nothing keeps its flat tensors alive and nobody shares a step count with a member that moves on."""
        for q, (mv, vv) in zip(st["params"], st["views"]):
            if self.state.get(q, {}).get("exp_avg") is mv and self.state[q].get("step") is st["step"]:
                s = st["step"].clone()
                self.state[q] = {"step": s, "exp_avg": mv.clone(), "exp_avg_sq": vv.clone()}
                self._t[q] = self._loose[q] = [s, st["cell"][1]]

    def _scaled_step(self, base):
        """grad_scale / found_inf are set: torch's step for everything.  The members of a run get a step tensor each for the
        duration (torch counts every list entry up, and down again on an inf); the flat moments are updated through their views."""
        live = []
        for key, st in list(self._runs.items()):
            if any(q.grad is None for q in st["params"]) or not self._bound(st):
                self._drop(self._runs.pop(key))      # its members will not step together
                continue
            steps = st["step"].expand(len(st["params"])).clone().unbind(0)
            for q, s in zip(st["params"], steps):
                self.state[q]["step"] = s
            live.append((st, steps))
        for c in self._loose.values():
            c[1] = None          # whether the step counts is decided on the device
        try:
            base(self)
        finally:
            for st, steps in live:
                st["step"].copy_(steps[0])
                st["cell"][1] = None
                for q in st["params"]:
                    self.state[q]["step"] = st["step"]

    def state_dict(self):
        """torch's layout, with a step tensor per parameter: a loader (a plain torch.optim.Adam) counts each entry up on its own."""
        sd = super().state_dict()
        sd["state"] = {k: ({**s, "step": s["step"].clone()} if torch.is_tensor(s.get("step")) else s) for k, s in sd["state"].items()}
        return sd

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        base = torch.optim.Adam.step
        if getattr(base, "hooked", False):   # the class-level hook wrapper of a plain torch Adam created elsewhere: this step's own wrapper runs the hooks
            base = base.__wrapped__
        if getattr(self, "grad_scale", None) is not None or getattr(self, "found_inf", None) is not None:
            self._scaled_step(base)
            return loss
        hidden, used = [], set()
        for gi, group in enumerate(self.param_groups):
            if (group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable")
                    or isinstance(group["lr"], torch.Tensor)):
                continue
            b1, b2 = group["betas"]
            for run in self._find_runs(group["params"], self._count):
                key = (gi, id(run[0]), len(run))
                st = self._run_state(key, run)
                used.add(key)
                st["cell"][1] += 1
                st["step"].add_(1.0)
                p0 = run[0]
                call("mmskin_adam_step", p0.data_ptr(), p0.grad.data_ptr(), ptr(st["m"]), ptr(st["v"]), st["n"], float(group["lr"]),
                     float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), st["cell"][1], stream())
                torch.autograd.graph.increment_version(run)       # the library wrote the parameters: version counters as after an in-place op
                for q in run:
                    hidden.append((q, q.grad)); q.grad = None     # torch's step skips parameters without a gradient
        for key in [k for k in self._runs if k not in used]:      # rebuilt under another key, or its members have no gradient now
            self._drop(self._runs.pop(key))
        try:
            base(self)
            for q, c in self._loose.items():                      # torch stepped them if they had a gradient
                if c[1] is not None and q.grad is not None:
                    c[1] += 1
        finally:
            for q, g in hidden:
                q.grad = g
        return loss
