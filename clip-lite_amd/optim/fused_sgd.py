"""Update path on the HIP kernels: global-norm clipping + SGD(momentum, weight decay, one group per tensor) + Lookahead
in one pass over the flat parameter arena (csrc/update_ops.hip).

Mirrors the reference objects: torch.optim.SGD built with one param group per parameter (reference factories.py:464-482)
wrapped in optim/lookahead.py:35-101's Lookahead(k, alpha). `state_dict()` keeps torch.optim.SGD's layout
(`momentum_buffer` per parameter), and — like the reference (lookahead.py:68-78) — the slow weights are not serialized but
re-seeded from the fast weights on load.
"""
import bisect
import ctypes as C
from typing import Any, Callable, Dict

import torch

from .. import hip

CHUNK = 8192     # elements per workgroup of the update kernel


class _FusedUpdate(torch.optim.Optimizer):
    """What the four fused optimizers share: the arena and the flat state buffers, the work-item table, global-norm clipping, the `hp` upload,
    launch(span) and the torch-compatible checkpoint layout. A class adds its `hp` length and tail, its state buffers and the kernels it enqueues."""
    HP_LEN = 8          # floats of `hp` (layout: csrc/update_ops.hip)
    STATE = {}          # checkpoint key -> flat state buffer (attribute name; f32, one element per arena element)

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        plist = [p for g in self.param_groups for p in g["params"]]
        arenas = {id(p._clite[0]) for p in plist if hasattr(p, "_clite")}
        if len(arenas) != 1 or any(not hasattr(p, "_clite") for p in plist):
            raise RuntimeError(f"{type(self).__name__}: parameters must live in one device arena — move the model to the GPU (model.to(device)) "
                               "before building the optimizer, as reference train.py:136-138 does")
        self.arena = plist[0]._clite[0]
        dev = self.arena.device
        for name in self.STATE.values():
            setattr(self, name, torch.zeros(self.arena.total, device=dev, dtype=torch.float32))
        self.flat_slow = self.arena.flat_p.clone()
        self.hp = torch.zeros(self.HP_LEN, device=dev, dtype=torch.float32)
        self.sumsq = torch.zeros(1, device=dev, dtype=torch.float32)
        self.sumsq_partials = torch.zeros(1024, device=dev, dtype=torch.float32)      # clite_sumsq's fixed-order first stage
        self.max_norm = 0.0
        self.grad_prescale = 1.0
        self._items = None
        self._hp_ring = None
        self._items_key = None
        self.before_step: Callable = None     # hook: e.g. wait for the gradient all-reduce stream

    # -- work-item table (one entry per <= CHUNK slice of one tensor) ------------------------------------------------
    def _base_lrs(self):
        return tuple((g.get("initial_lr", g["lr"]), g["weight_decay"], bool(g["params"][0].requires_grad)) for g in self.param_groups)

    def _build_items(self):
        key = self._base_lrs()
        if key == self._items_key:
            return
        rows = []
        for g, (lr, wd, on) in zip(self.param_groups, key):
            if not on:
                continue
            for p in g["params"]:
                o, n = self.arena.index[p._clite[1]]
                n4 = (n + 3) // 4 * 4
                for s in range(0, n4, CHUNK):
                    rows.append((o + s, min(CHUNK, n4 - s), lr, wd, self._reserved(p)))
        # frozen tensors: no work item, so the update kernel never zeroes their slice of flat_g — yet several backward kernels write
        # gradients unconditionally (BatchNorm dgamma/dbeta, LayerNorm, embeddings). Their (merged) spans are zeroed explicitly.
        spans = []
        for g, (_, _, on) in zip(self.param_groups, key):
            if on:
                continue
            for p in g["params"]:
                o, n = self.arena.index[p._clite[1]]
                if spans and spans[-1][1] == o:
                    spans[-1][1] = o + n
                else:
                    spans.append([o, o + n])
        self._frozen_spans = [tuple(x) for x in spans]
        rows.sort()                      # by arena offset: a [lo, hi) element range of the arena is then a contiguous run of items (launch(span=...))
        arr = (hip.OptimItem * len(rows))()
        for i, (s, c, lr, wd, tag) in enumerate(rows):
            arr[i].start, arr[i].count, arr[i].lr, arr[i].wd, arr[i].reserved = s, c, lr, wd, tag
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self._items = host.to(self.arena.device)
        self._n_items = len(rows)
        self._item_starts = [r[0] for r in rows]
        self._items_key = key

    def _reserved(self, p):
        """The `reserved` word of the items of parameter p (0: no kernel reads it)."""
        return 0

    def _lr_mult(self):
        for g in self.param_groups:
            base = g.get("initial_lr", None)
            if base:
                return g["lr"] / base
        return 1.0

    # -- reference train.py:222-223 ---------------------------------------------------------------------------------
    def clip_grad_norm(self, max_norm):
        """torch.nn.utils.clip_grad_norm_ over every parameter: the squared norm is reduced now, the scaling is applied
        inside the update kernel. Returns the (device) total norm of the pre-scaled gradients."""
        self.max_norm = float(max_norm)
        self.arena.join()
        self._build_items()
        self.zero_frozen()           # stale / unconditional gradients of frozen tensors must not enter the norm
        self.sumsq.zero_()
        self.sumsq_spans()
        return self.sumsq.sqrt() * self.grad_prescale

    def norm_spans(self):
        """The spans the squared gradient norm is summed over, in the FIXED order every path - eager, one graph, per-phase graphs - adds them into
        `sumsq` (so that all of them derive bit-identical clip factors): what is final before the image encoder's last weight-gradient groups (the text
        encoder, then layer3 .. the loss heads), then the late span (stem, layer1, layer2). The captured per-phase step sums the early spans on the main
        stream while the side stream finishes the late span's gradients (train_loop.TrainStep: norm_early); one span when the model has no such layout."""
        if getattr(self, "_norm_spans", None) is None:
            A = self.arena
            spans = [(0, A.total)]
            try:
                img, l3 = A.region("image_encoder."), A.region("image_encoder.img_encoder.layer3.")
                if img[0] < l3[0] < img[1]:
                    spans = [sp for sp in ((0, img[0]), (l3[0], A.total), (img[0], l3[0])) if sp[1] > sp[0]]
            except AssertionError:
                pass
            self._norm_spans = spans
        return self._norm_spans

    def sumsq_spans(self, part=None):
        """sumsq += the squared norm of the spans of `part`: None all, "early" all but the last, "late" the last (a single-span layout is all "late")."""
        spans = self.norm_spans()
        sel = spans if part is None else (spans[:-1] if part == "early" else spans[-1:])
        for lo, hi in sel:
            hip.sumsq(self.arena.flat_g[lo:hi], hi - lo, self.sumsq, self.sumsq_partials)

    def zero_grad(self, set_to_none: bool = False):
        """Gradients are zeroed by the update kernel itself; this only clears a backward that was not followed by step()."""
        self.arena.join()
        if getattr(self, "_dirty", True):
            self.arena.flat_g.zero_()
        self._dirty = True

    @torch.no_grad()
    def step(self, closure=None, lookahead_sync=False, alpha=1.0):
        if self.before_step is not None:
            self.before_step()
        self.upload_hp(lookahead_sync, alpha)
        self.launch()
        self.max_norm = 0.0
        return None

    # step() = upload_hp() + launch(). A captured hipGraph of the train step contains only launch() (and the sumsq of
    # clip_grad_norm); the host uploads this step's hyper-parameters into `hp` before every replay.
    def upload_hp(self, lookahead_sync=False, alpha=1.0, max_norm=None):
        """Host -> device: (lr multiplier of the schedule, momentum / beta1, clip norm, Lookahead sync flag, alpha, gradient pre-scale), then the
        class's own slots (_hp_tail)."""
        g0 = self.param_groups[0]
        mn = self.max_norm if max_norm is None else float(max_norm)
        self._upload([self._lr_mult(), g0["momentum"] if "momentum" in g0 else g0["betas"][0], mn, 1.0 if lookahead_sync else 0.0, alpha,
                      self.grad_prescale] + self._hp_tail())

    def _hp_tail(self):
        """What a class appends to the six common floats of `hp` (slots 6 ..; the rest of `hp` is zero)."""
        return []

    def _upload(self, vals):
        """`vals` (padded with zeros to the length of `hp`) -> device `hp`, without a host synchronisation in the steady state."""
        vals = list(vals) + [0.0] * (self.hp.numel() - len(vals))
        if not self.hp.is_cuda:
            self.hp.copy_(torch.tensor(vals))
            return
        # asynchronous upload from a small ring of pinned slots: a slot is rewritten only after the copy that read it has executed
        if self._hp_ring is None:
            self._hp_ring = [(torch.empty(self.hp.numel(), dtype=torch.float32).pin_memory(), torch.cuda.Event()) for _ in range(8)]
            self._hp_used = [False] * 8
            self._hp_next = 0
        i = self._hp_next
        self._hp_next = (i + 1) % len(self._hp_ring)
        host, ev = self._hp_ring[i]
        if self._hp_used[i]:
            ev.synchronize()
        host.copy_(torch.tensor(vals))
        self.hp.copy_(host, non_blocking=True)
        ev.record()
        self._hp_used[i] = True

    def zero_frozen(self):
        for lo, hi in getattr(self, "_frozen_spans", ()):
            self.arena.flat_g[lo:hi].zero_()

    def _launch_range(self, span):
        """What every launch() does first; returns (first item, number of items) of `span` (None: the whole table)."""
        self.arena.join()
        self._build_items()
        self.zero_frozen()
        first, n = 0, self._n_items
        if span is not None:
            first = bisect.bisect_left(self._item_starts, span[0])
            n = bisect.bisect_left(self._item_starts, span[1]) - first
        return first, n

    @torch.no_grad()
    def launch(self, span=None):
        """span = (lo, hi): update only the tensors whose arena offset lies in [lo, hi) — the captured step updates the image encoder at the end
        of a step and the rest at the start of the next one (train_loop.TrainStep, defer_update); every tensor exactly once per step."""
        first, n = self._launch_range(span)
        if n > 0:
            self._enqueue(C.c_void_p(self._items.data_ptr() + first * C.sizeof(hip.OptimItem)), first, n)
        self.arena._tr_stale = True          # the bf16 weights changed: the transposed copies of the dgrad GEMMs are out of date
        self._dirty = False

    def _enqueue(self, items, first, n):
        """The class's kernels over the n items from `items` on (item `first` of the table)."""
        raise NotImplementedError

    # -- checkpoints in the layout of the torch optimizer the class mirrors: STATE's keys per parameter, plus `step` where the class counts steps ----
    def state_dict(self):
        self.arena.flush_pending()          # a deferred share of the last update (TrainStep defer_update) must land before the state is read
        state, groups = {}, []
        for i, g in enumerate(self.param_groups):
            p = g["params"][0]
            o, n = self.arena.index[p._clite[1]]
            state[i] = {"step": torch.tensor(float(self.steps))} if hasattr(self, "steps") else {}
            state[i].update((k, self.arena._torch_view(getattr(self, buf), o, n, p).clone()) for k, buf in self.STATE.items())
            groups.append({k: v for k, v in g.items() if k != "params"} | {"params": [i]})
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        self.arena.flush_pending()
        for i, g in enumerate(self.param_groups):
            saved = sd["param_groups"][i]
            for k, v in saved.items():
                if k != "params":
                    g[k] = tuple(v) if k == "betas" else v
            p = g["params"][0]
            o, n = self.arena.index[p._clite[1]]
            st = sd["state"].get(i, sd["state"].get(str(i))) or {}
            for k, buf in self.STATE.items():
                if st.get(k) is not None:
                    self.arena._torch_view(getattr(self, buf), o, n, p).copy_(st[k])
            if hasattr(self, "steps") and st.get("step") is not None:
                self.steps = int(float(st["step"]))
        self._items_key = None


class FusedSGD(_FusedUpdate):
    """torch.optim.SGD with momentum and weight decay, one param group per parameter (clite_sgd_step); `state_dict()` keeps its layout
    (`momentum_buffer` per parameter)."""
    STATE = {"momentum_buffer": "flat_v"}

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0, nesterov=False))

    def _enqueue(self, items, first, n):
        hip.sgd_step(self.arena.flat_p, self.arena.flat_g, self.flat_v, self.flat_slow, self.arena.flat_lp, items, n, self.hp, self.sumsq)


class _PerTensorNorms:
    """What the layer-wise optimizers (FusedLARS, FusedLAMB) share: a norm slot per trainable tensor of two or more dimensions, the `reserved` word
    of that tensor's items (slot + 1; 0 = not adapted: biases, normalisation scales), and the buffers of the two-stage norm reduction."""

    def _init_norms(self):
        plist = [p for g in self.param_groups for p in g["params"]]
        adapted = [p for p in plist if p.dim() >= 2]
        self._slots = {id(p): i for i, p in enumerate(adapted)}
        dev = self.arena.device
        self.norms = torch.zeros(max(len(adapted), 1), 2, device=dev, dtype=torch.float32)      # a pair of squared norms per adapted tensor
        n_items = sum(((self.arena.index[p._clite[1]][1] + 3) // 4 * 4 + CHUNK - 1) // CHUNK for p in plist)
        self.norm_partials = torch.zeros(2 * max(n_items, 1), device=dev, dtype=torch.float32)  # the reduction's first stage: a pair per item

    def _reserved(self, p):
        return self._slots.get(id(p), -1) + 1

    def _partials(self, first, n):
        """Every span has its own share of the partials: two spans may be in flight on two streams (TrainStep: update_img / update_rest)."""
        return self.norm_partials[2 * first:2 * (first + n)]

    def tensor_norms(self, p):
        """The two norms of an adapted parameter as the last launch that updated it measured them."""
        return tuple(self.norms[self._slots[id(p)]].double().sqrt().tolist())


class FusedLARS(_PerTensorNorms, FusedSGD):
    """LARS (You, Gitman, Ginsburg 2017; the update SimCLR-style recipes run at batch sizes of 1k .. 32k) on FusedSGD's arena, work items, clipping,
    Lookahead hook, captured-step protocol and checkpoint layout (torch SGD's `momentum_buffer`, which is what LARS wrappers around torch.optim.SGD
    save): for every trainable tensor of two or more dimensions the SGD gradient term g' + wd p is scaled by the trust ratio
    trust_coefficient |p| / (|g'| + wd |p| + eps), where g' is the pre-scaled, clipped gradient (1 where either norm is zero); biases and
    normalisation scales (ndim <= 1) move exactly as under FusedSGD. The per-tensor norms are two launches over the item table
    (clite_lars_norms: fixed order, no float atomics), the update one (clite_lars_step); launch(span) takes the norms of the span it updates.
    tensor_norms(p) is (|p|, |g|), of the raw gradient: before pre-scale and clipping."""
    HP_LEN = 8          # FusedSGD's six, [6] the trust coefficient, [7] eps

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, trust_coefficient=0.001, eps=1e-8):
        super().__init__(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self.trust_coefficient, self.eps = float(trust_coefficient), float(eps)
        self._init_norms()

    def _hp_tail(self):
        return [self.trust_coefficient, self.eps]

    def _enqueue(self, items, first, n):
        A = self.arena
        hip.lars_norms(A.flat_p, A.flat_g, items, n, self._partials(first, n), self.norms)
        hip.lars_step(A.flat_p, A.flat_g, self.flat_v, self.flat_slow, A.flat_lp, items, n, self.hp, self.sumsq, self.norms)


class FusedAdamW(_FusedUpdate):
    """torch.optim.AdamW (reference factories.py:439, `OPTIM.OPTIMIZER_NAME: adamw`, torch's default betas / eps) on the same arena, work items, clipping,
    Lookahead hook and captured-step protocol as FusedSGD (clite_adamw_step). `state_dict()` keeps torch.optim.AdamW's layout (step, exp_avg, exp_avg_sq
    per parameter). The step count - the bias corrections' exponent - advances once per upload_hp(), i.e. once per optimizer step however many span
    launches the captured step splits it into."""
    HP_LEN = 12
    STATE = {"exp_avg": "flat_v", "exp_avg_sq": "flat_v2"}

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.steps = 0

    def upload_hp(self, lookahead_sync=False, alpha=1.0, max_norm=None):
        self.steps += 1
        super().upload_hp(lookahead_sync, alpha, max_norm)

    def _hp_tail(self):
        """[6] beta2, [7] eps, [8] 1 - beta1^t, [9] 1 - beta2^t, [10] 1 - beta1, [11] 1 - beta2, formed in double as torch does."""
        b1, b2 = self.param_groups[0]["betas"]
        return [b2, self.param_groups[0]["eps"], 1.0 - b1 ** self.steps, 1.0 - b2 ** self.steps, 1.0 - b1, 1.0 - b2]

    def _enqueue(self, items, first, n):
        hip.adamw_step(self.arena.flat_p, self.arena.flat_g, self.flat_v, self.flat_v2, self.flat_slow, self.arena.flat_lp, items, n, self.hp, self.sumsq)


class FusedLAMB(_PerTensorNorms, FusedAdamW):
    """LAMB (You et al. 2020, "Large Batch Optimization for Deep Learning", Algorithm 2) on FusedAdamW's moments, step counter, clipping, Lookahead
    hook, captured-step protocol and checkpoint layout (torch.optim.AdamW's step / exp_avg / exp_avg_sq): with r = m^ / (sqrt(v^) + eps) + wd p
    from this step's bias-corrected moments, every trainable tensor of two or more dimensions moves by lr q r, q = |p| / |r| (1 where either norm
    is zero; capped at 1 with trust_clip), biases and normalisation scales (ndim <= 1) exactly as under FusedAdamW. Bias correction is always on;
    there is no eps in q and no trust coefficient. Two launches per span: clite_lamb_moments (moments in place, the per-tensor norms in a fixed
    order, no float atomics) and clite_lamb_step. tensor_norms(p) is (|p| before the update, |r|)."""
    HP_LEN = 16          # FusedAdamW's twelve, [12] the TRUST_CLIP flag

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, trust_clip=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.trust_clip = bool(trust_clip)
        self._init_norms()

    def _hp_tail(self):
        return super()._hp_tail() + [1.0 if self.trust_clip else 0.0]

    def trust_ratio(self, p):
        """q of an adapted parameter in the last launch that updated it."""
        pn, rn = self.tensor_norms(p)
        q = pn / rn if pn > 0 and rn > 0 else 1.0
        return min(q, 1.0) if self.trust_clip else q

    def _enqueue(self, items, first, n):
        A = self.arena
        hip.lamb_moments(A.flat_p, A.flat_g, self.flat_v, self.flat_v2, items, n, self.hp, self.sumsq, self._partials(first, n), self.norms)
        hip.lamb_step(A.flat_p, A.flat_g, self.flat_v, self.flat_v2, self.flat_slow, A.flat_lp, items, n, self.hp, self.sumsq, self.norms)


class Lookahead(object):
    r"""Reference optim/lookahead.py:8-127 on top of FusedSGD: every ``k``-th step ``p = alpha*p + (1-alpha)*slow; slow = p`` —
    executed inside the same update kernel."""

    def __init__(self, optimizer: FusedSGD, k: int = 5, alpha: float = 0.8):
        self.optimizer = optimizer
        self.k = k
        self.alpha = alpha
        self._k_counter = 0
        self.optimizer.flat_slow.copy_(self.optimizer.arena.flat_p)     # slow weights start as a copy of the parameters

    def __getstate__(self):
        return {"optimizer": self.optimizer, "alpha": self.alpha, "k": self.k, "_k_counter": self._k_counter}

    @property
    def param_groups(self):
        return self.optimizer.param_groups

    @property
    def state(self):
        return self.optimizer.state

    def clip_grad_norm(self, max_norm):
        return self.optimizer.clip_grad_norm(max_norm)

    def zero_grad(self):
        self.optimizer.zero_grad()

    def state_dict(self):
        return self.optimizer.state_dict()

    def load_state_dict(self, state_dict: Dict[str, Any]):
        self.optimizer.load_state_dict(state_dict)
        self.optimizer.flat_slow.copy_(self.optimizer.arena.flat_p)      # reference lookahead.py:73-78

    def advance(self) -> bool:
        """Count one fast step; True when this step ends with the slow-weight synchronisation (reference lookahead.py:88-101)."""
        self._k_counter += 1
        sync = self._k_counter >= self.k
        if sync:
            self._k_counter = 0
        return sync

    def step(self, closure: Callable = None):
        return self.optimizer.step(closure, lookahead_sync=self.advance(), alpha=self.alpha)

    def load_slow_weights(self):
        a = self.optimizer.arena
        a.flush_pending()          # a deferred share of the last update must land on the FAST weights, not on top of the slow ones
        self._backup = a.flat_p.clone()
        a.flat_p.copy_(self.optimizer.flat_slow)
        a.refresh_lowp()

    def restore_fast_weights(self):
        a = self.optimizer.arena
        a.flush_pending()
        a.flat_p.copy_(self._backup)
        del self._backup
        a.refresh_lowp()
