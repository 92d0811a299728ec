"""Device-side helpers of the GEMM element tests: operands placed inside larger
NaN-filled buffers (leading dimension beyond the extent, base off the
allocator's alignment), C inside a buffer whose padding carries a bit pattern
that is compared after every call, a NaN-filled workspace, and the route
queries."""
import ctypes
import os

import numpy as np
import torch

PATTERN = 0x7FC12345                               # a quiet NaN with a payload
SLACK = 8                                          # elements after every operand
ROUTE_ENV = ("SCVAE_CD_WAVES", "SCVAE_CD_STEADY", "SCVAE_CG_FWD2",
             "SCVAE_GEMM_SPLIT_MIN_K")


def assert_default_routes():
    """The route assertions mean the default: no route-steering switch is set."""
    for name in ROUTE_ENV:
        assert name not in os.environ, name


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Placed:
    """A [rows, cols] operand at element `off` of a 1-D buffer, pitch cols + extra."""

    def __init__(self, rows, cols, dtype, device, extra=0, off=0, fill=float("nan")):
        self.rows, self.cols, self.ld, self.off = rows, cols, cols + extra, off
        n = off + rows * self.ld + SLACK
        self.buf = torch.full((n,), fill, dtype=dtype, device=device)
        self.view = self.buf[off:off + rows * self.ld].view(rows, self.ld)[:, :cols]
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + off * self.buf.element_size())

    def set(self, t):
        self.view.copy_(t)
        return self


def place(t, extra=0, off=0, fill=float("nan")):
    """t: a 2-D tensor on the device (or a NumPy array, uploaded to `cuda:0`)."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0")
    return Placed(t.shape[0], t.shape[1], t.dtype, t.device, extra, off, fill).set(t)


def place_u16(x, extra=0, off=0):
    """Counts as uint16 (carried as int16 bit patterns), padding 65535."""
    bits = np.ascontiguousarray(x).astype(np.uint16).view(np.int16)
    return place(bits, extra, off, fill=-1)


class Out:
    """C [M, N] inside a pattern-filled buffer; `take()` returns the result after
    checking that no byte outside [M, N] changed."""

    def __init__(self, M, N, device, extra=0, off=0, c0=None):
        self.p = Placed(M, N, torch.int32, device, extra, off, fill=PATTERN)
        self.mask = torch.zeros_like(self.p.buf, dtype=torch.bool)
        self.mask[off:off + M * self.p.ld].view(M, self.p.ld)[:, :N] = True
        if c0 is not None:
            self.p.view.copy_(c0.view(torch.int32))
        self.before = self.p.buf.clone()
        self.ptr, self.ld = self.p.ptr, self.p.ld

    def take(self):
        torch.cuda.synchronize()
        changed = (self.p.buf != self.before) & ~self.mask
        assert not bool(changed.any()), "bytes outside C changed at {}".format(
            changed.nonzero()[:4].flatten().tolist())
        return self.p.view.contiguous().view(torch.float32).cpu().numpy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.p.buf == self.before).all())


def workspace(nbytes, device):
    """NaN-filled, 256-byte aligned."""
    return torch.full((max(nbytes, 16) // 4 + 4,), float("nan"), device=device)


def gemm_route(lib, ta, tb, M, N, K, ldb, ws_bytes):
    out = (ctypes.c_int32 * 4)()
    assert lib.scvae_gemm_route(ta, tb, M, N, K, ldb, ws_bytes, out) == 0
    return tuple(out)


def count_route(lib, mode, rows, cols, N, u16, indexed):
    out = (ctypes.c_int32 * 8)()
    assert lib.scvae_count_gemm_route(mode, rows, cols, N, u16, indexed, out) == 0
    return tuple(out)[:7]


def run_gemm(lib, ta, tb, A, B, bias, M, N, K, relu=False, c0=None, use_ws=True,
             c_extra=0, c_off=0, want_route=None):
    """A, B, bias: Placed (bias may be None).  c0: a device [M, N] tensor to
    accumulate onto.  Returns C as NumPy."""
    from scvae_amd import _lib
    dev = A.buf.device
    ws_bytes = lib.scvae_gemm_workspace_bytes(M, N, K) if use_ws else 0
    if want_route is not None:
        assert gemm_route(lib, ta, tb, M, N, K, B.ld, ws_bytes) == want_route
    ws = workspace(ws_bytes, dev) if use_ws else None
    out = Out(M, N, dev, c_extra, c_off, c0)
    _lib.check(lib.scvae_gemm(
        ta, tb, A.ptr, B.ptr, bias.ptr if bias is not None else None, out.ptr, M, N, K,
        A.ld, B.ld, out.ld, 1 if relu else 0, 1 if c0 is not None else 0,
        ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, ws_bytes, stream()),
        "scvae_gemm")
    return out.take()


COUNT_ENTRIES = ("f32", "u16", "rows")


def run_count(lib, entry, mode, x, rows, cols, other, N, bias=None, relu=False,
              c_extra=0, c_off=0, x_rows=None):
    """x: Placed (fp32 for "f32", int16 bit patterns for "u16"; for "rows" the
    resident matrix, with x_rows the device int64 index)."""
    from scvae_amd import _lib
    dev = other.buf.device
    M = rows if mode == 0 else cols
    nbytes = lib.scvae_count_gemm_workspace_bytes(mode, rows, cols, N)
    assert nbytes >= 0
    ws = workspace(nbytes, dev)
    out = Out(M, N, dev, c_extra, c_off)
    args = [mode, x.ptr, x.ld, rows, cols, other.ptr, other.ld, N,
            bias.ptr if bias is not None else None, 1 if relu else 0, out.ptr, out.ld,
            ctypes.c_void_p(ws.data_ptr()), nbytes]
    if entry == "rows":
        args.append(ctypes.c_void_p(x_rows.data_ptr()))
    fn = {"f32": lib.scvae_count_gemm, "u16": lib.scvae_count_gemm_u16,
          "rows": lib.scvae_count_gemm_u16_rows}[entry]
    _lib.check(fn(*args, stream()), "scvae_count_gemm " + entry)
    return out.take()
