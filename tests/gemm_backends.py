"""The two ways a case of tests/gemm_exact.py reaches the engine, both through the C ABI of include/clite.h: numpy buffers and the wave-simulator
build (tests/simlib.py), torch device tensors and the gfx950 library (clip_lite_amd.hip). Both expose
  run(built)             uploads every allocation, sets the case's modes, makes its calls, restores the modes;
                         returns ([return codes], {output allocation: float32 values of the WHOLE allocation afterwards})
  set_tile_policy(p)     clite_set_tile_policy
The simulator backend adds dispatch(built): the launch log of a dry run of the case's calls."""
import ctypes as C

import numpy as np

from gemm_exact import BF16, Ref


def _fill(struct, fields, addr):
    for k, v in fields.items():
        setattr(struct, k, addr(v) if isinstance(v, Ref) else v)
    return struct


class _Backend:
    """Epilogue, Conv, Item: the ctypes mirrors of clite_epilogue, clite_conv, clite_wgrad_item; lib: the loaded library; stream(): hipStream_t"""

    def marshal(self, args, addr, keep):
        out = []
        for a in args:
            if isinstance(a, Ref):
                out.append(C.c_void_p(addr(a)))
            elif isinstance(a, tuple) and a[0] == "conv":
                keep.append(self.Conv(*a[1]))
                out.append(C.byref(keep[-1]))
            elif isinstance(a, tuple) and a[0] == "ep":
                keep.append(_fill(self.Epilogue(), a[1], addr))
                out.append(C.byref(keep[-1]))
            else:
                out.append(a)
        return out

    def call(self, entry, args, addr):
        if entry == "clite_wgrad_group":
            return self.group(args[0], args[1][1], addr)
        keep = []
        return getattr(self.lib, entry)(*self.marshal(args, addr, keep), self.stream())

    def items(self, members, addr):
        arr = (self.Item * len(members))()
        for it, m in zip(arr, members):
            for k, v in m.items():
                setattr(it, k, self.Conv(*v) if k == "cv" else addr(v) if isinstance(v, Ref) else v)
        return arr

    def run(self, b):
        case = b.case
        mem = {name: self.upload(kind, data) for name, (kind, data, _) in b.allocs.items()}
        addr = lambda r: self.address(mem[r.name], r.off)
        self.set_modes(case.get("det", 0), case.get("split", 0))
        try:
            rcs = [self.call(entry, args, addr) for entry, args in b.calls]
            got = {name: self.download(mem[name]) for name in b.expect}
        finally:
            self.set_modes(0, 0)
        return rcs, got


class SimBackend(_Backend):
    name = "wavesim"

    def __init__(self):
        import simlib
        self.s, self.lib = simlib, simlib.lib()
        self.Epilogue, self.Conv = simlib.Epilogue, simlib.Conv

        class Item(C.Structure):
            _fields_ = [("kind", C.c_int32), ("a", C.c_void_p), ("b", C.c_void_p), ("out", C.c_void_p), ("cv", simlib.Conv),
                        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32),
                        ("a_scales", C.c_void_p), ("b_scales", C.c_void_p), ("row_scale", C.c_void_p)]
        self.Item = Item
        self.lib.clite_wgrad_group.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        self.lib.clite_wgrad_group_workspace.argtypes = [C.c_int, C.c_int64, C.c_void_p]
        self._dummy = np.zeros(1 << 16, np.uint8)

    def stream(self):
        return None

    def upload(self, kind, data):
        return self.s.to_bf16(data) if kind == BF16 else data.copy()

    def address(self, m, off):
        return m.ctypes.data + off * m.itemsize

    def download(self, m):
        return self.s.from_bf16(m) if m.dtype == np.uint16 else m.copy()

    def set_modes(self, det, split):
        self.lib.clite_set_deterministic(int(det))
        self.lib.clite_set_f32_split(int(split))

    def set_tile_policy(self, p):
        assert self.lib.clite_set_tile_policy(int(p)) == 0

    def group(self, dt, members, addr):
        arr = self.items(members, addr)
        nb = C.c_uint64(0)
        assert self.lib.clite_wgrad_group_workspace(len(members), 1 << 14, C.byref(nb)) == 0
        ws_dev, ws_host = np.zeros(nb.value, np.uint8), np.zeros(nb.value, np.uint8)
        return self.lib.clite_wgrad_group(dt, arr, len(members), self.s.ptr(ws_dev), self.s.ptr(ws_host), nb.value, None)

    def dispatch(self, b):
        """the case's calls in DRY RUN (a launch is logged and returns without executing; no launcher dereferences an operand):
        ([return codes], [(kernel instantiation, (grid x, y, z), block x)])"""
        addr = lambda r: self._dummy.ctypes.data
        case = b.case
        self.set_modes(case.get("det", 0), case.get("split", 0))
        self.s.set_dry_run(True)
        self.s.clear_launch_log()
        try:
            rcs = [self.call(entry, args, addr) for entry, args in b.calls]
        finally:
            self.s.set_dry_run(False)
            self.set_modes(0, 0)
        return rcs, self.s.launch_log()


class HipBackend(_Backend):
    name = "hip"

    def __init__(self):
        import torch
        from clip_lite_amd import hip
        self.t, self.hip, self.lib = torch, hip, hip.lib()
        self.Epilogue, self.Conv, self.Item = hip.Epilogue, hip.Conv, hip.WgradItem

    def stream(self):
        return self.hip.stream_ptr()

    def upload(self, kind, data):
        x = self.t.from_numpy(data).to("cuda")
        return x.to(self.t.bfloat16) if kind == BF16 else x

    def address(self, m, off):
        return m.data_ptr() + off * m.element_size()

    def download(self, m):
        return m.float().cpu().numpy()

    def set_modes(self, det, split):
        self.hip.set_deterministic(bool(det))
        self.hip.set_f32_split(bool(split))

    def set_tile_policy(self, p):
        self.hip.set_tile_policy(p)

    def group(self, dt, members, addr):
        arr = self.items(members, addr)
        nb = C.c_uint64(0)
        self.hip.check(self.lib.clite_wgrad_group_workspace(len(members), 1 << 14, C.byref(nb)), "wgrad_group_workspace")
        ws_dev = self.t.empty(nb.value, dtype=self.t.uint8, device="cuda")
        ws_host = self.t.empty(nb.value, dtype=self.t.uint8).pin_memory()
        rc = self.lib.clite_wgrad_group(dt, arr, len(members), ws_dev.data_ptr(), ws_host.data_ptr(), nb.value, self.stream())
        self.t.cuda.synchronize()          # the pinned staging is read by a copy that is only enqueued
        return rc
