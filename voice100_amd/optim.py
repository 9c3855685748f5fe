"""Adam as the reference's models configure it (voice100/models/asr.py:169-176, tts.py:132-135, 239-241), one kernel launch per
step for the whole model (csrc/adam.hip).  A regular torch.optim.Optimizer -- param_groups, state_dict, LR schedulers
(StepLR in asr.py:175) all work -- whose step() runs on the HIP library when every parameter is a float32 CUDA tensor and
falls back to nothing else: CPU parameters raise (use torch.optim.Adam there; the product path is the GPU).

Gradient clipping as the reference's recipes ask for it (trainer.gradient_clip_val: torch.nn.utils.clip_grad_norm_ / clip_grad_value_
between backward and step) runs inside the same launch: FusedAdam.step(max_grad_norm=... | grad_clip_value=...), after one launch that
writes per-chunk partial norms.  clip_grad_norm_ / clip_grad_value_ below are the stand-alone form for any other optimizer."""
import math

import numpy as np
import torch

from . import _native as N


RING = 32


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = None
        self._partials = None          # per-chunk partial norms of every group, at fixed offsets (norm clipping)
        self.last_grad_norm = None     # total gradient norm of the last step that clipped by norm (0-dim device tensor)

    # The device-side tables (flat moment buffers, pointer arrays, step counter) are a cache of self.state / param_groups:
    # anything that replaces those -- load_state_dict() after a step has run (in-place resume, roll-back to a checkpoint),
    # add_param_group() -- drops the cache, and the next step() rebuilds it from self.state (keeping the loaded moments).
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._tables = None

    def _build(self, group):
        ps = [p for p in group["params"] if p.requires_grad]
        if not ps:
            return None
        dev = ps[0].device
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise RuntimeError("FusedAdam: parameters must be contiguous float32 CUDA tensors on one device")
        n = sum(p.numel() for p in ps)
        flat_m = torch.zeros(n, dtype=torch.float32, device=dev)
        flat_v = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        m_ptrs, v_ptrs, p_ptrs = [], [], []
        for p in ps:
            k = p.numel()
            st = self.state[p]
            if "exp_avg" in st:                              # resumed from a state_dict: keep its moments
                flat_m[off:off + k].copy_(st["exp_avg"].reshape(-1))
                flat_v[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
            st["exp_avg"] = flat_m[off:off + k].view_as(p)
            st["exp_avg_sq"] = flat_v[off:off + k].view_as(p)
            st.setdefault("step", torch.tensor(0.0))
            m_ptrs.append(flat_m.data_ptr() + 4 * off)
            v_ptrs.append(flat_v.data_ptr() + 4 * off)
            p_ptrs.append(p.data_ptr())
            off += k
        chunks, nchunks = _chunk_table([p.numel() for p in ps], dev)
        t = {"params": ps, "chunks": chunks, "nchunks": nchunks, "p": _to_dev(np.array(p_ptrs, dtype=np.uint64), dev),
             "m": _to_dev(np.array(m_ptrs, dtype=np.uint64), dev), "v": _to_dev(np.array(v_ptrs, dtype=np.uint64), dev),
             "g": _PtrTable(len(ps), dev), "flat": (flat_m, flat_v), "step": 0, "p_ptrs": p_ptrs}
        t["step"] = int(max(float(self.state[p]["step"]) for p in ps))
        return t

    def _upload_grads(self, t):
        """Point t["g"] (the device table of gradient pointers the partials and Adam kernels read) at this step's gradients."""
        ps = t["params"]
        grads = [p.grad for p in ps]
        f32 = torch.float32
        try:
            # one pass: a gradient that is not a contiguous fp32 CUDA tensor (None included) takes the slow path below
            bad = [i for i, g in enumerate(grads) if g.dtype is not f32 or not g.is_contiguous() or not g.is_cuda]
        except AttributeError:
            raise RuntimeError("FusedAdam: every parameter needs a gradient each step (the reference's models produce one)") from None
        for i in bad:
            grads[i] = ps[i].grad = grads[i].to(device=ps[i].device, dtype=f32).contiguous()
        if [p.data_ptr() for p in ps] != t["p_ptrs"]:        # every step: far cheaper than a write into freed memory
            raise RuntimeError("FusedAdam: a parameter's storage moved since the optimizer was built (re-create the optimizer)")
        t["g"].update([g.data_ptr() for g in grads])
        return grads

    @torch.no_grad()
    def step(self, closure=None, *, max_grad_norm=None, norm_type=2.0, grad_clip_value=None):
        """One Adam step of every parameter.  max_grad_norm: clip the gradients first as torch.nn.utils.clip_grad_norm_(all the
        optimizer's parameters, max_grad_norm, norm_type) would -- the norm spans every param group -- and leave the clipped gradients in
        p.grad; the total norm is then self.last_grad_norm (a 0-dim device tensor).  grad_clip_value: clip as clip_grad_value_ instead.
        No host synchronisation either way.  Without either argument the step is the plain one-launch-per-group update."""
        if max_grad_norm is not None and grad_clip_value is not None:
            raise ValueError("FusedAdam.step: pass max_grad_norm or grad_clip_value, not both")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._tables is None:
            self._tables = [self._build(g) for g in self.param_groups]
            self._partials = None
        live = [(group, t) for group, t in zip(self.param_groups, self._tables) if t is not None]
        grads = [self._upload_grads(t) for _, t in live]
        self.last_grad_norm = None
        if max_grad_norm is not None and live:
            mode, clip, code = CLIP_NORM, float(max_grad_norm), _norm_code(norm_type)
            if self._partials is None:
                self._partials = torch.empty(sum(t["nchunks"] for _, t in live), dtype=torch.float64, device=live[0][1]["chunks"].device)
            base = self._partials.data_ptr()
            for _, t in live:             # every group's partials before any group's update: the norm spans all of them
                N.call("v100_grad_norm_partials", t["chunks"], t["nchunks"], t["g"].dev, base, code)
                base += 8 * t["nchunks"]
            self.last_grad_norm = torch.empty((), dtype=torch.float32, device=self._partials.device)
            partials, npartials = self._partials, self._partials.numel()
        elif grad_clip_value is not None:
            mode, clip, code, partials, npartials = CLIP_VALUE, float(grad_clip_value), NORM_L2, None, 0
        else:
            mode = None
        for gi, (group, t) in enumerate(live):
            ps = t["params"]
            t["step"] += 1
            b1, b2 = group["betas"]
            if mode is None:
                N.call("v100_adam_step", t["chunks"], t["nchunks"], t["p"], t["g"].dev, t["m"], t["v"], float(group["lr"]), float(b1),
                       float(b2), float(group["eps"]), float(group["weight_decay"]), t["step"])
            else:
                N.call("v100_adam_step_clip", t["chunks"], t["nchunks"], t["p"], t["g"].dev, t["m"], t["v"], float(group["lr"]), float(b1),
                       float(b2), float(group["eps"]), float(group["weight_decay"]), t["step"], mode, clip, partials, npartials, code,
                       self.last_grad_norm if gi == 0 else None)
                torch.autograd.graph.increment_version(grads[gi])
            # the kernel wrote the parameters through raw pointers: advance their version counters (host-side metadata), or everything
            # keyed on them -- the eval-mode caches of folded coefficients / 16-bit weight copies -- would keep serving the old weights
            torch.autograd.graph.increment_version(ps)
            # state[p]["step"]: ONE host tensor shared by the group's parameters (attached once, advanced in place) -- what torch's
            # Adam keeps per parameter, without 170 dictionary writes a step
            st = t.get("step_tensor")
            if st is None or any(self.state[p].get("step") is not st for p in ps[:1]):
                st = t["step_tensor"] = torch.tensor(float(t["step"]))
                for p in ps:
                    self.state[p]["step"] = st
            else:
                st.fill_(float(t["step"]))
        return loss


# codes of include/voice100_hip.h (gradient clipping)
NORM_L2, NORM_INF = 2, -1
CLIP_NORM, CLIP_VALUE = 1, 2


def _norm_code(norm_type):
    nt = float(norm_type)
    if nt == 2.0:
        return NORM_L2
    if nt == math.inf:
        return NORM_INF
    raise ValueError(f"norm_type must be 2.0 or inf (the norms the HIP kernels compute), got {norm_type!r}")


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def _chunk_table(numels, dev):
    """(device array of {int tensor, int count, long long offset} records cutting every tensor into pieces of at most
    v100_adam_chunk_elems() elements, number of records): one workgroup per record in the Adam and clipping kernels."""
    ce = N.helper("v100_adam_chunk_elems")
    rec = np.array([(ti, min(ce, k - o), o) for ti, k in enumerate(numels) for o in range(0, k, ce)],
                   dtype=np.dtype([("tensor", "<i4"), ("count", "<i4"), ("offset", "<i8")]))
    return _to_dev(rec, dev), len(rec)


class _PtrTable:
    """Device array of tensor addresses (8 bytes each), re-uploaded only when they change: autograd hands out fresh gradient tensors
    every step, but the caching allocator usually hands back the same blocks, so most steps upload nothing."""

    def __init__(self, n, dev):
        self.dev = torch.empty(8 * n, dtype=torch.uint8, device=dev)
        # pinned staging buffers, used round-robin; an event per buffer says when its async copy has executed, and is waited for before
        # the buffer is rewritten RING uploads later (a no-op unless the host runs more than RING steps ahead of the GPU: with four slots
        # that wait was 0.55 ms of every step's 2.6 ms of enqueue time in a GPU-bound loop -- back-pressure, not work; 32 slots of 1.3 KB
        # keep it out of the enqueue path)
        self.ring = [torch.empty(8 * n, dtype=torch.uint8).pin_memory() for _ in range(RING)]
        self.events = [None] * RING
        self.pos = 0
        self.ptrs = None

    def update(self, ptrs):
        if ptrs == self.ptrs:
            return
        slot = self.pos % RING
        self.pos += 1
        host = self.ring[slot]
        if self.events[slot] is not None:
            self.events[slot].synchronize()
        host.numpy().view(np.uint64)[:] = ptrs
        self.dev.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[slot] = ev
        self.ptrs = ptrs


_clip_tables = {}


def _grad_tables(grads):
    """Chunk table, gradient-pointer table and partials buffer for this list of gradients, cached on their sizes."""
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev:
            raise RuntimeError("voice100_amd gradient clipping takes contiguous float32 CUDA gradients on one device")
    key = (dev, tuple(g.numel() for g in grads))
    t = _clip_tables.get(key)
    if t is None:
        if len(_clip_tables) >= 8:
            _clip_tables.clear()
        chunks, n = _chunk_table(key[1], dev)
        t = _clip_tables[key] = {"chunks": chunks, "nchunks": n, "g": _PtrTable(len(grads), dev),
                                 "partials": torch.empty(n, dtype=torch.float64, device=dev)}
    t["g"].update([g.data_ptr() for g in grads])
    return t


def _grads(parameters):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    return [p.grad for p in parameters if p.grad is not None and p.grad.numel()]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ for float32 CUDA gradients in two launches (per-chunk partial norms; then the total, the
    coefficient min(max_norm / (total + 1e-6), 1) and the in-place scale) and no host synchronisation.  Returns the total norm as a
    0-dim device tensor.  norm_type: 2.0 or inf."""
    code = _norm_code(norm_type)
    grads = _grads(parameters)
    if not grads:
        return torch.tensor(0.0)
    t = _grad_tables(grads)
    N.call("v100_grad_norm_partials", t["chunks"], t["nchunks"], t["g"].dev, t["partials"], code)
    if error_if_nonfinite and not bool(torch.isfinite(t["partials"]).all()):   # every partial finite <=> the total is
        raise RuntimeError(
            f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be clipped. To "
            "disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    total = torch.empty((), dtype=torch.float32, device=grads[0].device)
    N.call("v100_grad_clip", t["chunks"], t["nchunks"], t["g"].dev, CLIP_NORM, float(max_norm), t["partials"], t["nchunks"], code, total)
    torch.autograd.graph.increment_version(grads)
    return total


@torch.no_grad()
def clip_grad_value_(parameters, clip_value):
    """torch.nn.utils.clip_grad_value_ for float32 CUDA gradients: clamp to [-clip_value, clip_value] in place, one launch."""
    grads = _grads(parameters)
    if not grads:
        return
    t = _grad_tables(grads)
    N.call("v100_grad_clip", t["chunks"], t["nchunks"], t["g"].dev, CLIP_VALUE, float(clip_value), None, 0, NORM_L2, None)
    torch.autograd.graph.increment_version(grads)
