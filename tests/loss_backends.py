"""The two ways the shared checks of tests/loss_ref.py reach a kernel: numpy buffers through the wave simulator (tests/simlib.py), torch device
tensors through clip_lite_amd.hip. Both expose
  dev(array, kind)   numpy -> the backend's storage; kind 0 = bf16, 1 = f32, "i32", "i64"; None stays None
  host(handle)       storage -> numpy (bf16 widened to float32, which is exact)
  call(name, *args)  the C entry clite_<name> with the arguments in the C order (without the stream); returns 0 or the entry's -1."""
import ctypes as C

import numpy as np

BF16, F32 = 0, 1
_V, _I, _F, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64
SIGNATURES = {
    "critic_jsd_fwd": [_I, _V, _V, _V, _I, _I, _V, _V, _V],
    "critic_jsd_bwd": [_I, _V, _V, _V, _V, _V, _F, _I, _I, _V, _V, _V, _V, _V],
    "l2_normalize": [_I, _V, _V, _I, _I],
    "l2_normalize_bwd": [_I, _V, _V, _V, _V, _I, _I],
    "infonce_fwd": [_V, _I, _I, _V, _V, _V, _V],
    "infonce_bwd": [_I, _V, _I, _I, _V, _V, _V, _V, _F, _V, _I, _V],
    "prior_tail_fwd": [_I, _V, _V, _V, _I, _I, _I, _V, _V],
    "prior_tail_bwd": [_I, _V, _V, _V, _V, _F, _I, _I, _V, _V, _V],
    "loss_finalize": [_V, _F, _V],
    "add": [_I, _V, _V, _V, _U64],
    "xent_fwd": [_V, _I, _I, _I, _V, _I, _V, _V],
    "xent_bwd": [_I, _V, _I, _I, _I, _I, _V, _V, _V, _V, _V, _I],
}


class SimBackend:
    name = "wavesim"

    def __init__(self):
        import simlib
        self.s = simlib
        self.L = simlib.lib()
        for n, sig in SIGNATURES.items():
            getattr(self.L, "clite_" + n).argtypes = sig + [_V]

    def dev(self, a, kind):
        if a is None:
            return None
        if kind == BF16:
            return self.s.to_bf16(np.asarray(a, np.float32)).reshape(np.shape(a))
        return np.array(a, {F32: np.float32, "i32": np.int32, "i64": np.int64}[kind])

    def host(self, h):
        return self.s.from_bf16(h) if h.dtype == np.uint16 else h.copy()

    def call(self, name, *args):
        return getattr(self.L, "clite_" + name)(*[self.s.ptr(a) if isinstance(a, np.ndarray) else a for a in args], None)

    def set_deterministic(self, on):
        self.L.clite_set_deterministic(int(on))


class HipBackend:
    name = "hip"

    def __init__(self):
        import torch
        from clip_lite_amd import hip
        self.t, self.hip = torch, hip
        h = hip
        self.adapt = {          # C argument order -> the wrapper's
            "critic_jsd_fwd": lambda dt, f1, f2, t, B, D, neg, work, acc: h.critic_jsd_fwd(dt, f1, f2, t, B, D, work, acc, neg=neg),
            "critic_jsd_bwd": lambda dt, f1, f2, t, work, g, scale, B, D, neg, ninv, df1, df2, dtemp:
                h.critic_jsd_bwd(dt, f1, f2, t, work, g, scale, B, D, df1, df2, dtemp, neg=neg, neg_inv=ninv),
            "prior_tail_fwd": lambda dt, h1, w2, b2, B, K, sp, logit, acc: h.prior_tail_fwd(dt, h1, w2, b2, B, K, logit, acc, softplus=bool(sp)),
            "add": lambda dt, a, b, out, n: h.add(dt, a, b, out),
        }

    def dev(self, a, kind):
        if a is None:
            return None
        t = self.t
        if kind in (BF16, F32):
            x = t.from_numpy(np.array(a, np.float32)).to("cuda")
            return x.to(t.bfloat16) if kind == BF16 else x
        return t.from_numpy(np.array(a, np.int32 if kind == "i32" else np.int64)).to("cuda")

    def host(self, h):
        return (h.float() if h.dtype == self.t.bfloat16 else h).cpu().numpy()

    def call(self, name, *args):
        try:
            self.adapt.get(name, getattr(self.hip, name))(*args)
        except RuntimeError as e:
            if "failed with code -1" in str(e):          # hip.check on the C entry's refusal
                return -1
            raise
        return 0
