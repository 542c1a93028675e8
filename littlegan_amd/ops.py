"""torch-tensor front end of the C ABI (include/littlegan_hip.h).

PyTorch here is plumbing only: it owns device memory and the HIP stream.  Every function
validates shapes on the host (a wrong shape must never reach a hand-written kernel), then
enqueues the HIP kernels on torch's current stream.  No fallback paths.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import DT_BF16, DT_F32, check

_WS = {}
_WS_RETIRED = []     # buffers replaced by a bigger one after a HIP graph captured their address: kept alive for the replays
_WS_PINNED = False   # set by pin_workspaces() (EagerTrainer.graph_step) as soon as any graph holds workspace pointers
NSTAT = 8  # floats per sample in the instance-norm statistics record (lg_instnorm_stats_stride)


class Profile:
    """Optional per-launch HIP-event timing of the conv contractions (bench.py's live roofline leg).
    Events are recorded on torch's current stream = the stream the kernels are launched on."""
    enabled = False
    records = []  # (tag, algorithmic flops, start event, end event)
    after_conv = None  # bench.py's clock leg: called (no arguments) right behind every timed conv-class launch, on the launch stream

    @classmethod
    def start(cls):
        cls.records = []
        cls.enabled = True

    @classmethod
    def stop(cls):
        """-> {tag: (launches, total flops, total seconds)} ; call after a device synchronize"""
        cls.enabled = False
        out = {}
        for tag, fl, e0, e1 in cls.records:
            n, f, t = out.get(tag, (0, 0.0, 0.0))
            out[tag] = (n + 1, f + fl, t + e0.elapsed_time(e1) * 1e-3)
        cls.records = []
        return out


def _pb():
    if not Profile.enabled:
        return None
    _lib.load().lg_clear_kernel()   # lg_last_kernel is sticky: a launch path that names no kernel must not inherit the previous call's
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _pe(e0, tag, flops):
    """tag = class of the contraction (what the FLOP formula depends on) + the kernel template the C side really launched"""
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        kern = _lib.load().lg_last_kernel().decode() or tag   # unnamed launch path: filed under its class tag
        Profile.records.append((f"{tag}:{kern}", float(flops), e0, e1))
        if Profile.after_conv is not None:
            Profile.after_conv()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _chk(t, shape=None, name="tensor"):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous fp32 CUDA tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {tuple(shape)}")
    return t


def pin_workspaces():
    """Call before a HIP-graph capture: a captured graph holds the RAW addresses of the scratch buffers below, so from now on
    a buffer that is outgrown is retired (kept allocated) instead of being handed back to the caching allocator, where a
    later tensor could land under a replaying graph's writes."""
    global _WS_PINNED
    _WS_PINNED = True


def last_kernel() -> str:
    """Name of the kernel the most recent conv-class, dense or head C-ABI call launched on this thread (lg_last_kernel; sticky:
    lg_clear_kernel in front of a call whose route is to be read)."""
    return _lib.load().lg_last_kernel().decode()


def last_norm_launches():
    """[(kernel, gridDim.x, gridDim.y), ...] of the most recent instance-norm / dropout C-ABI call on this thread, in launch order
    (lg_instnorm_last_launches; [] if the call was refused before its first launch)."""
    s = _lib.load().lg_instnorm_last_launches().decode()
    out = []
    for item in filter(None, s.split(";")):
        name, _, grid = item.rpartition("[")
        gx, gy = grid.rstrip("]").split(",")
        out.append((name, int(gx), int(gy)))
    return out


def workspace(nbytes: int, device, tag="default") -> torch.Tensor:
    """Grow-only scratch buffer per (device, tag); kernels on one stream run in order so sharing is safe."""
    key = (str(device), tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and _WS_PINNED:
            _WS_RETIRED.append(buf)
        if torch.cuda.is_current_stream_capturing():
            raise _lib.LittleGanHipError(f"workspace '{tag}' must grow to {nbytes} bytes during a HIP-graph capture: run the "
                                         "step once eagerly at this shape first")
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


# ------------------------------------------------------------------ conv layers
def conv_pack_bytes(cb, cs, dtype):
    return int(_lib.load().lg_conv_pack_bytes(cb, cs, dtype))


def conv_pack(w, cb, cs, dtype, out=None):
    """w: master kernel [5,5,cb,cs] -> packed MFMA operand images (uint8 buffer)."""
    _chk(w, (5, 5, cb, cs), "w")
    if out is None:
        out = torch.empty(conv_pack_bytes(cb, cs, dtype), dtype=torch.uint8, device=w.device)
    check(_lib.load().lg_conv_pack(_p(w), _p(out), cb, cs, dtype, _stream()), "lg_conv_pack")
    return out


def conv2d_s2_fwd(x, pack, bias, cs, dtype, out=None):
    B, H, W, cb = x.shape
    _chk(x, name="x")
    if H % 2 or W % 2:
        raise ValueError("conv2d_s2_fwd: H and W must be even")
    if out is None:
        out = torch.empty(B, H // 2, W // 2, cs, dtype=torch.float32, device=x.device)
    _chk(out, (B, H // 2, W // 2, cs), "out")
    if bias is not None:
        _chk(bias, (cs,), "bias")
    e0 = _pb()
    check(_lib.load().lg_conv2d_s2_fwd(_p(x), _p(pack), _p(bias), _p(out), B, H // 2, W // 2, cb, cs, dtype, _stream()),
          "lg_conv2d_s2_fwd")
    _pe(e0, "conv_igemm_patch" if cb == 3 else "conv_igemm_down", 50.0 * B * (H // 2) * (W // 2) * cb * cs)
    return out


class NormPartials:
    """First-pass sums of an InstanceNormalization backward, produced by the epilogue of the conv that wrote the gradient
    (lg_*_dgrad_nf): `buf` holds [B][nparts][2] doubles.  Valid until the next fused data gradient is enqueued (one
    shared workspace; kernels of a stream run in order and the consumer is the very next norm backward)."""

    def __init__(self, buf, nparts, alpha, shape):
        self.buf, self.nparts, self.alpha, self.shape = buf, nparts, float(alpha), tuple(shape)


def _nf_args(fuse, B, up, Hs, Ws, N, device):
    """fuse = (z16, stats, alpha) of the layer the produced gradient belongs to -> ctypes arguments + result holder"""
    import ctypes
    z16, st, alpha = fuse
    if z16.dtype != torch.bfloat16 or not z16.is_contiguous() or z16.shape[0] != B:
        raise ValueError("fuse: z16 must be the contiguous bf16 conv output of the layer below")
    _chk(st, (B, NSTAT), "fuse stats")
    lib = _lib.load()
    ws = workspace(int(lib.lg_conv_stats_workspace_bytes(int(up), B, Hs, Ws, N)), device, "nfpart")
    return z16, st, float(alpha), ws, ctypes.c_int(0)


def conv2d_s2_dgrad(dy, pack, cb, dtype, out=None, dy16=None, out_bf16=False, fuse=None):
    """dx [B,2Hs,2Ws,cb]; out_bf16: return the gradient as a bf16 tensor (no fp32 copy is written).
    dy may be None when its bf16 mirror dy16 is given and the halo kernel covers the shape (conv_halo_supported).
    fuse = (z16, stats, alpha) (bf16 path, out_bf16): the kernel also writes the first-pass sums of the norm backward the
    gradient feeds; returns (dx, NormPartials or None)."""
    B, Hs, Ws, cs = (dy if dy is not None else dy16).shape
    if fuse is not None:
        import ctypes
        if not (out_bf16 and dy16 is not None and dtype == DT_BF16):
            raise ValueError("conv2d_s2_dgrad: fuse needs the bf16 path (dy16, out_bf16)")
        _chk16(dy16, dy16, "dy16")
        out = torch.empty(B, 2 * Hs, 2 * Ws, cb, dtype=torch.bfloat16, device=dy16.device)
        z16, st, alpha, ws, npo = _nf_args(fuse, B, True, Hs, Ws, cb, dy16.device)
        e0 = _pb()
        check(_lib.load().lg_conv2d_s2_dgrad_nf(_p(dy16), _p(pack), _p(out), B, Hs, Ws, cb, cs, _p(z16), _p(st), alpha, _p(ws),
                                               ws.numel(), ctypes.addressof(npo), _stream()), "lg_conv2d_s2_dgrad_nf")
        _pe(e0, "conv_igemm_up", 50.0 * B * Hs * Ws * cb * cs)
        return out, (NormPartials(ws, npo.value, alpha, out.shape) if npo.value > 0 else None)
    if dy is not None:
        _chk(dy, name="dy")
    if dy16 is not None:
        _chk16(dy16, dy if dy is not None else dy16, "dy16")
    if dtype != DT_BF16 and (dy is None or out_bf16):
        raise ValueError("conv2d_s2_dgrad: dtype f32 needs the fp32 gradient and writes fp32 (bf16 mirror / bf16 output: dtype bf16)")
    dev = (dy if dy is not None else dy16).device
    if out_bf16:
        out = torch.empty(B, 2 * Hs, 2 * Ws, cb, dtype=torch.bfloat16, device=dev)
        o32, o16 = None, out
    else:
        if out is None:
            out = torch.empty(B, 2 * Hs, 2 * Ws, cb, dtype=torch.float32, device=dev)
        _chk(out, (B, 2 * Hs, 2 * Ws, cb), "out")
        o32, o16 = out, None
    e0 = _pb()
    check(_lib.load().lg_conv2d_s2_dgrad_m16(_p(dy), _p(dy16), _p(pack), _p(o32), _p(o16), B, Hs, Ws, cb, cs, dtype, _stream()),
          "lg_conv2d_s2_dgrad_m16")
    _pe(e0, "conv_igemm_up_n3" if cb == 3 else "conv_igemm_up", 50.0 * B * Hs * Ws * cb * cs)
    return out


def _wgrad(fn_name, big, small, dw, accumulate, dtype, swap, big16=None, small16=None):
    lib = _lib.load()
    B, Hs, Ws, cs = (small if small is not None else small16).shape
    cb = (big if big is not None else big16).shape[3]
    if big is not None:
        _chk(big, (B, 2 * Hs, 2 * Ws, cb), "big")
    if small is not None:
        _chk(small, name="small")
    n3 = cb == 3 and big is not None and small16 is not None  # 3-channel layer: fp32 image + mirror of the wide operand
    if (big is None or small is None) and (big16 is None or small16 is None) and not n3:
        raise ValueError("wgrad: an fp32 operand may be omitted only when BOTH bf16 mirrors are given")
    _chk(dw, (5, 5, cb, cs), "dw")
    nbytes = int(lib.lg_wgrad_workspace_bytes(B, Hs, Ws, cb, cs, dtype))
    ws = workspace(nbytes, dw.device, "wgrad")
    if n3:
        big16 = None
        _chk16(small16, small if small is not None else small16, "small16")
    elif big16 is None or small16 is None:
        big16 = small16 = None  # the bf16-source kernel needs both mirrors
    else:
        _chk16(big16, big if big is not None else big16, "big16")
        _chk16(small16, small if small is not None else small16, "small16")
    (a, a16), (b, b16) = ((small, small16), (big, big16)) if swap else ((big, big16), (small, small16))
    e0 = _pb()
    check(getattr(lib, fn_name)(_p(a), _p(a16), _p(b), _p(b16), _p(dw), _p(ws), ws.numel(), B, Hs, Ws, cb, cs,
                                int(accumulate), dtype, _stream()), fn_name)
    _pe(e0, "wgrad_patch" if cb == 3 else "wgrad_igemm", 50.0 * B * Hs * Ws * cb * cs)
    return dw


def conv2d_s2_wgrad(x, dy, dw, accumulate, dtype, x16=None, dy16=None):
    """dw[5,5,cb,cs] (+)= wgrad(x [B,2Hs,2Ws,cb], dy [B,Hs,Ws,cs]); x16/dy16: optional bf16 mirrors"""
    return _wgrad("lg_conv2d_s2_wgrad_m16", x, dy, dw, accumulate, dtype, swap=False, big16=x16, small16=dy16)


def convT_s2_fwd(x, pack, bias, cb, dtype, out=None):
    B, Hs, Ws, cs = x.shape
    _chk(x, name="x")
    if out is None:
        out = torch.empty(B, 2 * Hs, 2 * Ws, cb, dtype=torch.float32, device=x.device)
    _chk(out, (B, 2 * Hs, 2 * Ws, cb), "out")
    if bias is not None:
        _chk(bias, (cb,), "bias")
    e0 = _pb()
    check(_lib.load().lg_convT_s2_fwd(_p(x), _p(pack), _p(bias), _p(out), B, Hs, Ws, cb, cs, dtype, _stream()),
          "lg_convT_s2_fwd")
    _pe(e0, "conv_igemm_up", 50.0 * B * Hs * Ws * cb * cs)
    return out


def convT_s2_dgrad(dy, pack, cs, dtype, out=None, dy16=None, out_bf16=False, fuse=None):
    """fuse: as conv2d_s2_dgrad -> returns (dx, NormPartials or None)"""
    B, H, W, cb = (dy if dy is not None else dy16).shape
    if fuse is not None:
        import ctypes
        if not (out_bf16 and dy16 is not None and dtype == DT_BF16):
            raise ValueError("convT_s2_dgrad: fuse needs the bf16 path (dy16, out_bf16)")
        _chk16(dy16, dy16, "dy16")
        out = torch.empty(B, H // 2, W // 2, cs, dtype=torch.bfloat16, device=dy16.device)
        z16, st, alpha, ws, npo = _nf_args(fuse, B, False, H // 2, W // 2, cs, dy16.device)
        e0 = _pb()
        check(_lib.load().lg_convT_s2_dgrad_nf(_p(dy16), _p(pack), _p(out), B, H // 2, W // 2, cb, cs, _p(z16), _p(st), alpha,
                                              _p(ws), ws.numel(), ctypes.addressof(npo), _stream()), "lg_convT_s2_dgrad_nf")
        _pe(e0, "conv_igemm_down", 50.0 * B * (H // 2) * (W // 2) * cb * cs)
        return out, (NormPartials(ws, npo.value, alpha, out.shape) if npo.value > 0 else None)
    if dy is not None:
        _chk(dy, name="dy")
    if dy16 is not None:
        _chk16(dy16, dy if dy is not None else dy16, "dy16")
    if dtype != DT_BF16 and (dy is None or out_bf16):
        raise ValueError("convT_s2_dgrad: dtype f32 needs the fp32 gradient and writes fp32 (bf16 mirror / bf16 output: dtype bf16)")
    dev = (dy if dy is not None else dy16).device
    if out_bf16:
        out = torch.empty(B, H // 2, W // 2, cs, dtype=torch.bfloat16, device=dev)
        o32, o16 = None, out
    else:
        if out is None:
            out = torch.empty(B, H // 2, W // 2, cs, dtype=torch.float32, device=dev)
        _chk(out, (B, H // 2, W // 2, cs), "out")
        o32, o16 = out, None
    e0 = _pb()
    check(_lib.load().lg_convT_s2_dgrad_m16(_p(dy), _p(dy16), _p(pack), _p(o32), _p(o16), B, H // 2, W // 2, cb, cs, dtype,
                                            _stream()), "lg_convT_s2_dgrad_m16")
    _pe(e0, "conv_igemm_down", 50.0 * B * (H // 2) * (W // 2) * cb * cs)
    return out


def convT_s2_dgrad_bn_supported(B, Hs, Ws, cb, cs, dtype):
    return dtype == DT_BF16 and bool(_lib.load().lg_convT_s2_dgrad_bn_supported(B, Hs, Ws, cb, cs))


def instnorm_bwd_coef(z16, stats, partials):
    """The norm backward WITHOUT its apply pass: per-sample records [B, 8] from the statistics and the producer-fused sums
    (NormPartials).  The consumer (convT_s2_dgrad_bn) forms dz while it stages its operand."""
    B = z16.shape[0]
    _chk(stats, (B, NSTAT), "stats")
    if tuple(z16.shape) != partials.shape:
        raise ValueError(f"instnorm_bwd_coef: partial sums were produced for shape {partials.shape}, got {tuple(z16.shape)}")
    coef = torch.empty(B, 8, dtype=torch.float32, device=z16.device)
    check(_lib.load().lg_instnorm_bwd_coef(_p(stats), _p(partials.buf), int(partials.nparts), _p(coef), B, z16.numel() // B, _stream()),
          "lg_instnorm_bwd_coef")
    return coef


def convT_s2_dgrad_bn(z16, g16, coef, alpha, pack, cs, fuse):
    """Data gradient of Conv2DTranspose(cb, 5, 2, same) from the level's raw pair (z16, g16) [B, 2Hs, 2Ws, cb] + coef
    (instnorm_bwd_coef): dz is formed on the fly.  fuse = (z16, stats, alpha) of the level below -> (dx16 [B, Hs, Ws, cs], NormPartials)."""
    import ctypes
    B, H, W, cb = z16.shape
    _chk16(z16, z16, "z16")
    _chk16(g16, z16, "g16")
    if tuple(g16.shape) != tuple(z16.shape):
        raise ValueError("convT_s2_dgrad_bn: z16 and g16 must have the same shape")
    _chk(coef, (B, 8), "coef")
    if not convT_s2_dgrad_bn_supported(B, H // 2, W // 2, cb, cs, DT_BF16):
        raise ValueError(f"convT_s2_dgrad_bn: unsupported shape B={B} {H // 2}x{W // 2} cb={cb} cs={cs}")
    out = torch.empty(B, H // 2, W // 2, cs, dtype=torch.bfloat16, device=z16.device)
    zl, stl, alpha_l, ws, npo = _nf_args(fuse, B, False, H // 2, W // 2, cs, z16.device)
    e0 = _pb()
    check(_lib.load().lg_convT_s2_dgrad_bn(_p(z16), _p(g16), _p(coef), float(alpha), _p(pack), _p(out), B, H // 2, W // 2, cb, cs,
                                          _p(zl), _p(stl), alpha_l, _p(ws), ws.numel(), ctypes.addressof(npo), _stream()),
          "lg_convT_s2_dgrad_bn")
    _pe(e0, "conv_igemm_down", 50.0 * B * (H // 2) * (W // 2) * cb * cs)
    if npo.value <= 0:
        raise _lib.LittleGanHipError("lg_convT_s2_dgrad_bn returned no partial sums")
    return out, NormPartials(ws, npo.value, alpha_l, out.shape)


def convT_s2_wgrad(x, dy, dw, accumulate, dtype, x16=None, dy16=None):
    """dw[5,5,cb,cs] (+)= wgrad(x [B,Hs,Ws,cs], dy [B,2Hs,2Ws,cb]); x16/dy16: optional bf16 mirrors"""
    return _wgrad("lg_convT_s2_wgrad_m16", dy, x, dw, accumulate, dtype, swap=True, big16=dy16, small16=x16)


def n3_m16_supported(H, W, cb, cs, dtype):
    """bf16 path: the 3-channel layers of this shape read the bf16 mirror of their wide operand alone."""
    return bool(_lib.load().lg_n3_m16_supported(H, W, cb, cs, dtype))


def convT_s1_tanh_fwd(x, pack, bias, cb, dtype, out=None, x16=None):
    """x16: bf16 mirror of x (bf16 path); x may be None where n3_m16_supported."""
    t = x if x is not None else x16
    B, H, W, cs = t.shape
    if x is not None:
        _chk(x, name="x")
    if x16 is not None:
        _chk16(x16, t, "x16")
    if out is None:
        out = torch.empty(B, H, W, cb, dtype=torch.float32, device=t.device)
    _chk(out, (B, H, W, cb), "out")
    _chk(bias, (cb,), "bias")
    e0 = _pb()
    check(_lib.load().lg_convT_s1_tanh_fwd_m16(_p(x), _p(x16), _p(pack), _p(bias), _p(out), B, H, W, cb, cs, dtype,
                                               _stream()), "lg_convT_s1_tanh_fwd_m16")
    _pe(e0, "conv_igemm_s1t_n3", 50.0 * B * H * W * cb * cs)
    return out


def convT_s1_tanh_fwd_z16_supported(H, W, cb, cs, dtype):
    return bool(_lib.load().lg_convT_s1_tanh_fwd_z16_supported(H, W, cb, cs, dtype))


def convT_s1_tanh_fwd_z16(z16, stats, alpha, pack, bias, cb, dtype, out=None):
    """The final layer fed with the RAW bf16 conv output z16 [B,H,W,cs] of the last decoder level and its statistics:
    InstanceNorm + LeakyReLU(alpha) happen while the kernel stages its input, the normalised map is never written."""
    B, H, W, cs = z16.shape
    _chk16(z16, z16, "z16")
    _chk(stats, (B, NSTAT), "stats")
    if out is None:
        out = torch.empty(B, H, W, cb, dtype=torch.float32, device=z16.device)
    _chk(out, (B, H, W, cb), "out")
    _chk(bias, (cb,), "bias")
    e0 = _pb()
    check(_lib.load().lg_convT_s1_tanh_fwd_z16(_p(z16), _p(stats), float(alpha), _p(pack), _p(bias), _p(out), B, H, W, cb, cs,
                                               dtype, _stream()), "lg_convT_s1_tanh_fwd_z16")
    _pe(e0, "conv_igemm_s1t_n3", 50.0 * B * H * W * cb * cs)
    return out


def convT_s1_tanh_bwd(x, dpre, pack, cs, dtype, dx=None, dw=None, db=None, accumulate=False, x16=None, dx16=None, fuse=None):
    """x16: bf16 mirror of x for the weight gradient; dx16: bf16 tensor that receives the data gradient instead of dx.
    fuse = (z16, stats, alpha) (with dx16): also the first-pass sums of the norm backward dx16 feeds -> returns
    (dx16, NormPartials or None)."""
    lib = _lib.load()
    B, H, W, cb = dpre.shape
    _chk(dpre, name="dpre")
    if x is not None:
        _chk(x, (B, H, W, cs), "x")
    if x16 is not None:
        if x16.dtype != torch.bfloat16 or tuple(x16.shape) != (B, H, W, cs) or not x16.is_contiguous():
            raise ValueError("convT_s1_tanh_bwd: x16 must be a contiguous bf16 [B,H,W,cs] tensor")
    if dx is not None:
        _chk(dx, (B, H, W, cs), "dx")
    if dx16 is not None:
        if dx16.dtype != torch.bfloat16 or tuple(dx16.shape) != (B, H, W, cs) or not dx16.is_contiguous():
            raise ValueError("convT_s1_tanh_bwd: dx16 must be a contiguous bf16 [B,H,W,cs] tensor")
    if dw is not None:
        _chk(dw, (5, 5, cb, cs), "dw")
    if db is not None:
        _chk(db, (cb,), "db")
    nbytes = int(lib.lg_convT_s1_bwd_workspace_bytes(B, H, W, cb, cs, dtype))
    ws = workspace(nbytes, dpre.device, "wgrad")
    if fuse is not None:
        import ctypes
        if dx16 is None or dx is not None:
            raise ValueError("convT_s1_tanh_bwd: fuse needs the bf16 data gradient (dx16)")
        z16, st, alpha, wsp, npo = _nf_args(fuse, B, False, H, W, cs, dpre.device)
        check(lib.lg_convT_s1_tanh_bwd_nf(_p(x), _p(x16), _p(dpre), _p(pack), _p(dx16), _p(dw), _p(db), _p(ws), ws.numel(), B, H, W,
                                          cb, cs, int(accumulate), dtype, _p(z16), _p(st), alpha, _p(wsp), wsp.numel(),
                                          ctypes.addressof(npo), _stream()), "lg_convT_s1_tanh_bwd_nf")
        return dx16, (NormPartials(wsp, npo.value, alpha, dx16.shape) if npo.value > 0 else None)
    check(lib.lg_convT_s1_tanh_bwd_m16(_p(x), _p(x16), _p(dpre), _p(pack), _p(dx), _p(dx16), _p(dw), _p(db), _p(ws),
                                       ws.numel(), B, H, W, cb, cs, int(accumulate), dtype, _stream()),
          "lg_convT_s1_tanh_bwd_m16")
    return dx if dx is not None else dx16


def bias_grad(dy, db, accumulate=False, dy16=None):
    """db (+)= column sums of dy [.., C]; dy16: bf16 copy read instead of dy (dy may then be None)"""
    t = dy if dy is not None else dy16
    C = t.shape[-1]
    M = t.numel() // C
    if dy is not None:
        _chk(dy, name="dy")
    if dy16 is not None:
        _chk16(dy16, t, "dy16")
    _chk(db, (C,), "db")
    lib = _lib.load()
    ws = workspace(int(lib.lg_bias_grad_workspace_bytes(M, C)), t.device, "small")
    check(lib.lg_bias_grad_m16(_p(dy), _p(dy16), _p(db), _p(ws), ws.numel(), M, C, int(accumulate), _stream()),
          "lg_bias_grad_m16")
    return db


_HALO_OK = {}


def conv_halo_supported(mode, dtype, B, Hm, Wm, Cs, N):
    """mode 0 = conv form ("down": M grid Hm x Wm is the SMALL map), 1 = convT form ("up").  Host-side query."""
    key = (mode, dtype, B, Hm, Wm, Cs, N)
    if key not in _HALO_OK:
        _HALO_OK[key] = bool(_lib.load().lg_conv_halo_supported(mode, dtype, B, Hm, Wm, Cs, N))
    return _HALO_OK[key]


# ------------------------------------------------------------------ instance norm
class Moments:
    """UNFINISHED InstanceNormalization moments of a conv output (bf16 activation path): the [B][nparts][3] partial records
    {count, mean, M2} the conv epilogue left in the shared 'statpart' workspace, and the [B, NSTAT] tensor the finished
    statistics go to.  The next norm call on this stream consumes them: instnorm_apply finishes them inside its own launch
    (lg_instnorm_leaky_apply_z16_p: one launch and one kernel boundary less per normalised map); any other use goes through
    stats_tensor(), which runs the stand-alone finalize.  Valid until the next conv with fused moments is enqueued."""

    def __init__(self, ws, nparts, gamma, beta, B):
        self.ws, self.nparts, self.gamma, self.beta, self.B = ws, int(nparts), gamma, beta, int(B)
        self.stats = torch.empty(B, NSTAT, dtype=torch.float32, device=ws.device)
        self.covered = 0   # rows whose records have been finished

    def __getitem__(self, rows):
        lo, hi, step = rows.indices(self.B)
        if step != 1:
            raise ValueError("Moments: contiguous row ranges only")
        return _MomentRows(self, lo, hi)


class _MomentRows:
    def __init__(self, m, lo, hi):
        self.m, self.lo, self.hi = m, lo, hi


def stats_tensor(st):
    """[B, NSTAT] statistics tensor of `st` (a tensor already, or Moments: finished here if no apply has done it)."""
    if isinstance(st, _MomentRows):
        return stats_tensor(st.m)[st.lo:st.hi]
    if not isinstance(st, Moments):
        return st
    if st.covered < st.B:
        check(_lib.load().lg_instnorm_stats_finalize(_p(st.ws), st.nparts, _p(st.stats), _p(st.gamma), _p(st.beta), st.B, _stream()),
              "lg_instnorm_stats_finalize")
        st.covered = st.B
    return st.stats


class Raw:
    """A level's output handed over UN-normalised: the raw bf16 conv output z [B,H,W,C] and its finished statistics
    records [B, NSTAT], standing for the map bf16(LeakyReLU(InstanceNorm(z))) that was never written.  The consumers that take one
    (instnorm_apply as a skip, convT_s2_fwd_stats_ns) normalise on the way in, bit-identically to reading the stored map."""
    __slots__ = ("z", "stats")

    def __init__(self, z, stats):
        if not (isinstance(z, torch.Tensor) and z.dtype == torch.bfloat16 and z.is_contiguous()):
            raise ValueError("Raw: z must be a contiguous bf16 tensor")
        _chk(stats, (z.shape[0], NSTAT), "Raw.stats")
        self.z, self.stats = z, stats

    @property
    def shape(self):
        return self.z.shape


def instnorm_stats(x, gamma, beta, pre_leaky, alpha, stats=None, x16_out=None):
    """x16_out (optional bf16 tensor like x): also receives bf16(x) in the same pass."""
    B = x.shape[0]
    Ln = x.numel() // B
    _chk(x, name="x")
    if stats is None:
        stats = torch.empty(B, NSTAT, dtype=torch.float32, device=x.device)
    _chk(stats, (B, NSTAT), "stats")
    lib = _lib.load()
    ws = workspace(int(lib.lg_instnorm_workspace_bytes(B, Ln)), x.device, "small")
    if x16_out is not None:
        _chk16(x16_out, x, "x16_out")
    check(lib.lg_instnorm_leaky_stats_z16(_p(x), _p(stats), _p(gamma), _p(beta), _p(ws), ws.numel(), B, Ln, int(pre_leaky),
                                          float(alpha), _p(x16_out), _stream()), "lg_instnorm_leaky_stats")
    return stats


def _chk16(t, like, name):
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and t.numel() == like.numel()):
        raise ValueError(f"{name}: need a contiguous bf16 CUDA tensor with {like.numel()} elements")
    return t


class Drop:
    """Dropout context of one encoder norm pass: `key` = the int64 [2] device tensor {seed, key_offset} of the step
    (a step input, like gp_eps), the call slot of the encoder pass within the step, the encoder level (1..4), the row the first
    sample of the tensor at hand has in that call's batch, and the rate.  The forward apply multiplies its output by keep * scale,
    the backward the arriving gradient; both regenerate the mask from these five values alone."""
    __slots__ = ("key", "call", "level", "r0", "rate")

    def __init__(self, key, call, level=1, r0=0, rate=0.5):
        if not (isinstance(key, torch.Tensor) and key.is_cuda and key.dtype == torch.int64 and key.numel() == 2 and key.is_contiguous()):
            raise ValueError("Drop: key must be a contiguous int64 CUDA tensor {seed, key_offset}")
        self.key, self.call, self.level, self.r0, self.rate = key, int(call), int(level), int(r0), float(rate)

    def at(self, level=None, r0=None):
        return Drop(self.key, self.call, self.level if level is None else level, self.r0 if r0 is None else r0, self.rate)

    @property
    def threshold(self):
        """T = round(rate * 65536) as the library rounds it (the rate crosses the C ABI as a float)"""
        import ctypes
        return int(round(ctypes.c_float(self.rate).value * 65536.0))

    @property
    def active(self):
        """False: the mask keeps everything (T == 0) and the pass is bit-identical to its plain twin"""
        return self.threshold > 0

    def _args(self):
        return (_p(self.key), self.call, self.level, self.r0, self.rate)


def _chk_drop(drop, what, skip, pre_leaky, post_leaky, Ln):
    if skip is not None or pre_leaky or not post_leaky:
        raise ValueError(f"{what}: dropout exists for the encoder's form only (no skip operand, pre_leaky=0, post_leaky=1)")
    if Ln % 8:
        raise ValueError(f"{what}: dropout needs a multiple of 8 elements per sample (one Philox block per 8 elements), got {Ln}")


def dropout_key(seed, key_offset, device="cuda", out=None):
    """The step's dropout key {seed, key_offset} as the int64 [2] device tensor the norm kernels read, written by a one-block
    kernel from launch scalars: no host-to-device copy, so the host does not wait for the stream."""
    if out is None:
        out = torch.empty(2, dtype=torch.int64, device=device)
    if not (out.is_cuda and out.dtype == torch.int64 and out.numel() == 2 and out.is_contiguous()):
        raise ValueError("dropout_key: out must be a contiguous int64 CUDA tensor of 2 elements")
    check(_lib.load().lg_dropout_key(_p(out), _i64(seed), _i64(key_offset), _stream()), "lg_dropout_key")
    return out


def dropout_mask(key, call, level, r0, B, L, rate):
    """keep [B, L] uint8 (1 = kept) of rows r0 .. r0+B-1 of the (call, level) slot: the mask definition, for tests and debugging"""
    d = Drop(key, call, level, r0, rate)
    keep = torch.empty(B, L, dtype=torch.uint8, device=key.device)
    check(_lib.load().lg_dropout_mask(_p(key), d.call, d.level, d.r0, B, L, d.rate, _p(keep), _stream()), "lg_dropout_mask")
    return keep


def instnorm_apply(x, stats, skip, pre_leaky, post_leaky, alpha, out=None, out16=None, want_f32=True, drop=None):
    """want_f32=False: only the bf16 mirror out16 is written (returns None).
    x may be the bf16 conv output of the bf16 activation path (then skip may be bf16 too).
    drop (ops.Drop, optional): the output is multiplied by the dropout mask's keep * scale (encoder form only); without it the code
    path and the launches are exactly the plain ones."""
    B = x.shape[0]
    Ln = x.numel() // B
    x_is16 = x.dtype == torch.bfloat16
    if x_is16:
        _chk16(x, x, "x")
        if Ln % 8:
            raise ValueError("instnorm_apply: a bf16 input needs a multiple of 8 elements per sample")
    else:
        _chk(x, name="x")
    if drop is not None:
        _chk_drop(drop, "instnorm_apply", skip, pre_leaky, post_leaky, Ln)
    pend = None   # unfinished moments (Moments / a row range of them): finished inside the apply launch where the kernel exists
    if isinstance(stats, (Moments, _MomentRows)):
        mrows = stats if isinstance(stats, _MomentRows) else _MomentRows(stats, 0, stats.B)
        if mrows.hi - mrows.lo != B:
            raise ValueError("instnorm_apply: moments cover a different number of samples")
        if x_is16 and not pre_leaky and mrows.m.covered < mrows.m.B:
            pend = mrows
            stats = mrows.m.stats[mrows.lo:mrows.hi]
        else:
            stats = stats_tensor(stats)
    _chk(stats, (B, NSTAT), "stats")
    raw_skip = skip if isinstance(skip, Raw) else None
    if raw_skip is not None:   # the skip is a raw (z, records) pair: normalised inside the launch (norm_rs.hip)
        if not x_is16 or pre_leaky or drop is not None:
            raise ValueError("instnorm_apply: a raw skip needs the bf16 input path, pre_leaky=0 and no dropout")
        if raw_skip.z.numel() != x.numel():
            raise ValueError("instnorm_apply: skip has a different size")
        skip = None
    skip16 = skip is not None and skip.dtype == torch.bfloat16
    if skip is not None:
        if skip16:
            if not x_is16:
                raise ValueError("instnorm_apply: a bf16 skip needs the bf16 input path")
            _chk16(skip, x, "skip")
        else:
            _chk(skip, name="skip")
        if skip.numel() != x.numel():
            raise ValueError("instnorm_apply: skip has a different size")
    if not want_f32:
        if out16 is None:
            raise ValueError("instnorm_apply: want_f32=False needs out16")
        out = None
    else:
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _chk(out, x.shape, "out")
    if out16 is not None:
        _chk16(out16, x, "out16")
    if drop is not None:
        lib = _lib.load()
        if pend is not None:
            m = pend.m
            part = m.ws.data_ptr() + pend.lo * m.nparts * 3 * 8
            check(lib.lg_instnorm_leaky_apply_z16_p_drop(_p(x), part, m.nparts, _p(m.gamma), _p(m.beta), _p(stats), _p(out), _p(out16), B, Ln,
                                                         float(alpha), *drop._args(), _stream()), "lg_instnorm_leaky_apply_z16_p_drop")
            m.covered += B
        elif x_is16:
            check(lib.lg_instnorm_leaky_apply_z16_drop(_p(x), _p(stats), _p(out), _p(out16), B, Ln, float(alpha), *drop._args(), _stream()),
                  "lg_instnorm_leaky_apply_z16_drop")
        else:
            check(lib.lg_instnorm_leaky_apply_drop(_p(x), _p(stats), _p(out), _p(out16), B, Ln, float(alpha), *drop._args(), _stream()),
                  "lg_instnorm_leaky_apply_drop")
        return out
    if raw_skip is not None:
        lib = _lib.load()
        if pend is not None:
            m = pend.m
            part = m.ws.data_ptr() + pend.lo * m.nparts * 3 * 8
            check(lib.lgadj_instnorm_apply_p_rs(_p(x), part, m.nparts, _p(m.gamma), _p(m.beta), _p(stats), _p(raw_skip.z),
                                                _p(raw_skip.stats), _p(out), _p(out16), B, Ln, int(post_leaky), float(alpha), _stream()),
                  "lgadj_instnorm_apply_p_rs")
            m.covered += B
        else:
            check(lib.lgadj_instnorm_apply_rs(_p(x), _p(stats), _p(raw_skip.z), _p(raw_skip.stats), _p(out), _p(out16), B, Ln,
                                              int(post_leaky), float(alpha), _stream()), "lgadj_instnorm_apply_rs")
        return out
    if pend is not None:
        m = pend.m
        part = m.ws.data_ptr() + pend.lo * m.nparts * 3 * 8
        check(_lib.load().lg_instnorm_leaky_apply_z16_p(_p(x), part, m.nparts, _p(m.gamma), _p(m.beta), _p(stats), _p(skip), int(skip16),
                                                        _p(out), _p(out16), B, Ln, int(post_leaky), float(alpha), _stream()),
              "lg_instnorm_leaky_apply_z16_p")
        m.covered += B
    elif x_is16:
        check(_lib.load().lg_instnorm_leaky_apply_z16(_p(x), _p(stats), _p(skip), int(skip16), _p(out), _p(out16), B, Ln,
                                                      int(pre_leaky), int(post_leaky), float(alpha), _stream()),
              "lg_instnorm_leaky_apply_z16")
    else:
        check(_lib.load().lg_instnorm_leaky_apply(_p(x), _p(stats), _p(skip), _p(out), _p(out16), B, Ln, int(pre_leaky),
                                                  int(post_leaky), float(alpha), _stream()), "lg_instnorm_leaky_apply")
    return out


def instnorm_bwd(x, stats, g, dgamma, dbeta, pre_leaky, post_leaky, alpha, accumulate=False, out=None, out16=None,
                 want_f32=True, db=None, partials=None, drop=None):
    """g may be fp32 or bf16 (as written by a bf16 data-gradient conv); x fp32, or the bf16 conv output of the bf16
    activation path.  Returns the fp32 dx (or None if want_f32 is False, in which case only the bf16 mirror out16 is
    written).  db [C] (optional, C = x.shape[-1]): receives the column sums of dx = the bias gradient of the conv
    layer that produced x, in the same pass.
    drop (ops.Drop, optional): g is multiplied by the dropout mask's keep * scale — the forward's, regenerated — in both passes of
    the backward (encoder form only); without it the code path and the launches are exactly the plain ones."""
    B = x.shape[0]
    Ln = x.numel() // B
    x_is16 = x.dtype == torch.bfloat16
    if x_is16:
        _chk16(x, x, "x")
        if Ln % 8:
            raise ValueError("instnorm_bwd: a bf16 input needs a multiple of 8 elements per sample")
    else:
        _chk(x, name="x")
    if drop is not None:
        _chk_drop(drop, "instnorm_bwd", None, pre_leaky, post_leaky, Ln)
        if partials is not None and drop.active:
            raise ValueError("instnorm_bwd: producer-fused partial sums are those of the unmasked gradient; with an active dropout "
                             "mask the first pass must run (partials=None)")
    g16 = g.dtype == torch.bfloat16
    if g16:
        _chk16(g, x, "g")
    else:
        _chk(g, name="g")
        if g.numel() != x.numel():
            raise ValueError("instnorm_bwd: g has a different size")
    _chk(stats, (B, NSTAT), "stats")
    if want_f32:
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _chk(out, x.shape, "out")
    else:
        if out16 is None:
            raise ValueError("instnorm_bwd: want_f32=False needs out16")
        out = None
    if out16 is not None:
        _chk16(out16, x, "out16")
    lib = _lib.load()
    C = 0
    if db is not None:
        C = x.shape[-1]
        _chk(db, (C,), "db")
    ws = workspace(int(lib.lg_instnorm_bwd_db_workspace_bytes(B, Ln, C)), x.device, "small")
    if partials is not None:  # NormPartials from the conv that produced g: the first pass over (x, g) is skipped
        if not x_is16:
            raise ValueError("instnorm_bwd: fused partial sums belong to the bf16 activation path")
        # the producer's store loop hard-codes g' = LeakyReLU'_alpha(a c + b) g (lg_nf_accum): anything else is another sum
        if pre_leaky or not post_leaky or float(alpha) != partials.alpha or tuple(x.shape) != partials.shape:
            raise ValueError(f"instnorm_bwd: partial sums were produced for the post-LeakyReLU(alpha={partials.alpha}) form on "
                             f"shape {partials.shape}; asked for pre={pre_leaky} post={post_leaky} alpha={alpha} shape {tuple(x.shape)}")
        if drop is not None:
            check(lib.lg_instnorm_leaky_bwd_z16_drop(_p(x), _p(stats), _p(g), int(g16), _p(out), _p(out16), _p(dgamma), _p(dbeta), _p(db), C,
                                                     _p(partials.buf), int(partials.nparts), _p(ws), ws.numel(), B, Ln, float(alpha),
                                                     int(accumulate), *drop._args(), _stream()), "lg_instnorm_leaky_bwd_z16_drop")
            return out
        check(lib.lg_instnorm_leaky_bwd_z16_p(_p(x), _p(stats), _p(g), int(g16), _p(out), _p(out16), _p(dgamma), _p(dbeta), _p(db), C,
                                              _p(partials.buf), int(partials.nparts), _p(ws), ws.numel(), B, Ln, int(pre_leaky),
                                              int(post_leaky), float(alpha), int(accumulate), _stream()),
              "lg_instnorm_leaky_bwd_z16_p")
        return out
    if drop is not None:
        if x_is16:
            check(lib.lg_instnorm_leaky_bwd_z16_drop(_p(x), _p(stats), _p(g), int(g16), _p(out), _p(out16), _p(dgamma), _p(dbeta), _p(db), C,
                                                     None, 0, _p(ws), ws.numel(), B, Ln, float(alpha), int(accumulate), *drop._args(),
                                                     _stream()), "lg_instnorm_leaky_bwd_z16_drop")
        else:
            check(lib.lg_instnorm_leaky_bwd_drop(_p(x), _p(stats), _p(g), int(g16), _p(out), _p(out16), _p(dgamma), _p(dbeta), _p(db), C,
                                                 _p(ws), ws.numel(), B, Ln, float(alpha), int(accumulate), *drop._args(), _stream()),
                  "lg_instnorm_leaky_bwd_drop")
        return out
    fn = lib.lg_instnorm_leaky_bwd_z16 if x_is16 else lib.lg_instnorm_leaky_bwd_db
    check(fn(_p(x), _p(stats), _p(g), int(g16), _p(out), _p(out16), _p(dgamma), _p(dbeta), _p(db), C, _p(ws), ws.numel(), B, Ln,
             int(pre_leaky), int(post_leaky), float(alpha), int(accumulate), _stream()), "lg_instnorm_leaky_bwd")
    return out


# ------------------------------------------------------------------ dense
def dense_fwd(x, w, bias, out=None):
    B, K = x.shape
    N = w.shape[1]
    _chk(x, name="x")
    _chk(w, (K, N), "w")
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    _chk(out, (B, N), "out")
    check(_lib.load().lg_dense_fwd(_p(x), _p(w), _p(bias), _p(out), B, K, N, _stream()), "lg_dense_fwd")
    return out


def dense_wgrad(x, dy, dw, db, accumulate=False):
    B, K = x.shape
    N = dy.shape[1]
    _chk(x, name="x")
    _chk(dy, (B, N), "dy")
    _chk(dw, (K, N), "dw")
    check(_lib.load().lg_dense_wgrad(_p(x), _p(dy), _p(dw), _p(db), B, K, N, int(accumulate), _stream()),
          "lg_dense_wgrad")


def concat_cols(a, c, out=None):
    """[a | c] along the last axis (the Generator's dense input, model.py:97-98)."""
    B, ka = a.shape
    kc = c.shape[1]
    _chk(a, name="a")
    _chk(c, (B, kc), "c")
    if out is None:
        out = torch.empty(B, ka + kc, dtype=torch.float32, device=a.device)
    _chk(out, (B, ka + kc), "out")
    check(_lib.load().lg_concat_cols(_p(a), ka, _p(c), kc, _p(out), B, _stream()), "lg_concat_cols")
    return out


def adj_conditions(first, second):
    """(t, u) = (concat([first, second], 0), (t + 1) * 0.5): the Adjuster's target / input conditions (eager_trainer.py:153-154)."""
    B, c = first.shape
    _chk(first, name="first")
    _chk(second, (B, c), "second")
    t = torch.empty(2 * B, c, dtype=torch.float32, device=first.device)
    u = torch.empty_like(t)
    check(_lib.load().lg_adj_conditions(_p(first), _p(second), _p(t), _p(u), B, c, _stream()), "lg_adj_conditions")
    return t, u


def dense_dgrad(dy, w, out=None):
    B, N = dy.shape
    K = w.shape[0]
    _chk(dy, name="dy")
    _chk(w, (K, N), "w")
    if out is None:
        out = torch.empty(B, K, dtype=torch.float32, device=dy.device)
    _chk(out, (B, K), "out")
    check(_lib.load().lg_dense_dgrad(_p(dy), _p(w), _p(out), B, K, N, _stream()), "lg_dense_dgrad")
    return out


def heads_fwd(x, wpr, bpr, wc, bc, out=None):
    B, K = x.shape
    c = wc.shape[1]
    _chk(x, name="x")
    _chk(wpr, (K, 1), "wpr")
    _chk(wc, (K, c), "wc")
    if out is None:
        out = torch.empty(B, 1 + c, dtype=torch.float32, device=x.device)
    _chk(out, (B, 1 + c), "out")
    lib = _lib.load()
    ws = workspace(int(lib.lg_heads_fwd_workspace_bytes(B, K, c)), x.device, "small")
    check(lib.lg_heads_fwd(_p(x), _p(wpr), _p(bpr), _p(wc), _p(bc), _p(out), _p(ws), ws.numel(), B, K, c, _stream()),
          "lg_heads_fwd")
    return out


def heads_dgrad(dz, wpr, wc, out=None):
    B = dz.shape[0]
    K, c = wc.shape
    _chk(dz, (B, 1 + c), "dz")
    if out is None:
        out = torch.empty(B, K, dtype=torch.float32, device=dz.device)
    _chk(out, (B, K), "out")
    check(_lib.load().lg_heads_dgrad(_p(dz), _p(wpr), _p(wc), _p(out), B, K, c, _stream()), "lg_heads_dgrad")
    return out


def heads_wgrad(x, dz, dwpr, dbpr, dwc, dbc, accumulate=False):
    B, K = x.shape
    c = dwc.shape[1]
    _chk(x, name="x")
    _chk(dz, (B, 1 + c), "dz")
    _chk(dwpr, (K, 1), "dwpr")
    _chk(dwc, (K, c), "dwc")
    check(_lib.load().lg_heads_wgrad(_p(x), _p(dz), _p(dwpr), _p(dbpr), _p(dwc), _p(dbc), B, K, c, int(accumulate),
                                     _stream()), "lg_heads_wgrad")


# ------------------------------------------------------------------ losses / optimizer
def bce_heads_loss(p, t_c, t_pr, w_pr, w_c, loss, dz, accumulate):
    B, J = p.shape
    _chk(p, name="p")
    _chk(dz, (B, J), "dz")
    if t_c is not None:
        _chk(t_c, (B, J - 1), "t_c")
    check(_lib.load().lg_bce_heads_loss_fwd_bwd(_p(p), _p(t_c), float(t_pr), float(w_pr), float(w_c), _p(loss), _p(dz),
                                                B, J - 1, int(accumulate), _stream()), "lg_bce_heads_loss_fwd_bwd")


# ------------------------------------------------------------------ logit-side objectives (objective.hip; include/littlegan_hip_obj.h)
GAN_ROLE_D_REAL, GAN_ROLE_D_FAKE, GAN_ROLE_G = 0, 1, 2


def heads_fwd_logit(x, wpr, bpr, wc, bc, out=None, z_out=None):
    """heads_fwd that also keeps the logit of output_pr: -> (p [B, 1 + c], bit for bit heads_fwd's; z_pr [B], the pre-sigmoid p[:, 0])"""
    B, K = x.shape
    c = wc.shape[1]
    _chk(x, name="x")
    _chk(wpr, (K, 1), "wpr")
    _chk(bpr, (1,), "bpr")
    _chk(wc, (K, c), "wc")
    _chk(bc, (c,), "bc")
    if out is None:
        out = torch.empty(B, 1 + c, dtype=torch.float32, device=x.device)
    if z_out is None:
        z_out = torch.empty(B, dtype=torch.float32, device=x.device)
    _chk(out, (B, 1 + c), "out")
    _chk(z_out, (B,), "z_out")
    lib = _lib.load()
    ws = workspace(int(lib.lg_heads_fwd_workspace_bytes(B, K, c)), x.device, "small")
    check(lib.lgo_heads_fwd(_p(x), _p(wpr), _p(bpr), _p(wc), _p(bc), _p(out), _p(z_out), _p(ws), ws.numel(), B, K, c, _stream()),
          "lgo_heads_fwd")
    return out, z_out


def gan_heads_loss(p, z_pr, t_c, kind, role, w_pr, w_c, loss, dz, accumulate):
    """bce_heads_loss with the real / fake term taken on the logit z_pr [B]: kind 1 logistic, 2 hinge, 3 lsgan, 4 wgan; role 0 D on real
    rows, 1 D on fake rows, 2 G / Adjuster.  The attribute term (t_c, w_c) is bce_heads_loss's."""
    B, J = p.shape
    _chk(p, name="p")
    _chk(z_pr, (B,), "z_pr")
    _chk(dz, (B, J), "dz")
    _chk(loss, (1,), "loss")
    if t_c is not None:
        _chk(t_c, (B, J - 1), "t_c")
    check(_lib.load().lgo_gan_heads_loss_fwd_bwd(_p(p), _p(z_pr), _p(t_c), int(kind), int(role), float(w_pr), float(w_c), _p(loss), _p(dz),
                                                 B, J - 1, int(accumulate), _stream()), "lgo_gan_heads_loss_fwd_bwd")


def l1_tanh_loss(t, img, g_in, dpre, loss, lam, accumulate):
    _chk(t, name="t")
    _chk(img, t.shape, "img")
    if g_in is not None:
        _chk(g_in, t.shape, "g_in")
    if dpre is not None:
        _chk(dpre, t.shape, "dpre")
    lib = _lib.load()
    ws = workspace(int(lib.lg_l1_workspace_bytes()), t.device, "small")
    check(lib.lg_l1_tanh_loss_fwd_bwd(_p(t), _p(img), _p(g_in), _p(dpre), _p(loss), _p(ws), ws.numel(), t.numel(),
                                      float(lam), int(accumulate), _stream()), "lg_l1_tanh_loss_fwd_bwd")


def _chk_counter(t, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.numel() == 1):
        raise ValueError(f"{name}: need a 1-element int32 CUDA tensor, got {t.dtype} {t.device} numel={t.numel()}")
    return t


def _chk_adam(who, state, *operands, ema_state=None):
    """The operand check of the six Adam wrappers (plain, sched_, guard_, each with and without the weight average) -> n.  operands: w, g,
    m, v and, for the passes that also update the average, ema (then ema_state is its counter).  state None: not checked, which is what
    clip_adam_update and sched_clip_adam_update, the two on the default step, have always done (DESIGN.md §33 has the cost of checking)."""
    n = operands[0].numel()
    for t, nm in zip(operands, ("w", "g", "m", "v", "ema")):
        _chk(t, name=nm)
        if t.numel() != n:
            raise ValueError(f"{who}: size mismatch")
    if state is not None:
        _chk(state, (2,), "state")
    if len(operands) == 5:
        _chk_counter(ema_state, "ema_state")
    return n


def clip_adam_update(w, g, m, v, state, lr, b1, b2, eps, clip, gscale=1.0):
    n = _chk_adam("clip_adam_update", None, w, g, m, v)
    check(_lib.load().lg_clip_adam_update(_p(w), _p(g), _p(m), _p(v), n, _p(state), float(lr), float(b1), float(b2),
                                          float(eps), float(clip), float(gscale), _stream()), "lg_clip_adam_update")


def adam_advance(state, b1, b2):
    check(_lib.load().lg_adam_advance(_p(state), float(b1), float(b2), _stream()), "lg_adam_advance")


def clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, ema_state, lr, b1, b2, eps, clip, gscale, decay):
    """clip + Adam on [lo, hi) of one model's weights `w` and the weight average `ema` over all of them (lo == hi: the average
    alone): ema -= (1 - d_t)(ema - w), d_t = min(decay, (1 + k) / (10 + k)), k = ema_state[0] (lg_clip_adam_ema_update)."""
    n = _chk_adam("clip_adam_ema_update", state, w, g, m, v, ema, ema_state=ema_state)
    check(_lib.load().lg_clip_adam_ema_update(_p(w), _p(g), _p(m), _p(v), _p(ema), n, int(lo), int(hi), _p(state), _p(ema_state),
                                              float(lr), float(b1), float(b2), float(eps), float(clip), float(gscale),
                                              float(decay), _stream()), "lg_clip_adam_ema_update")


def ema_advance(ema_state):
    check(_lib.load().lg_ema_advance(_p(_chk_counter(ema_state, "ema_state")), _stream()), "lg_ema_advance")


def swap_f32(a, b):
    """a <-> b in place (lg_swap_f32)."""
    _chk(a, name="a")
    _chk(b, a.shape, "b")
    check(_lib.load().lg_swap_f32(_p(a), _p(b), a.numel(), _stream()), "lg_swap_f32")


# ------------------------------------------------------------------ conv forward with fused InstanceNorm moments
def _fwd_stats(fn_name, x, x16, pack, bias, out, B, Hs, Ws, cb, cs, dtype, gamma, beta, tag, flops, up, defer=False):
    """Runs the conv (`out` fp32, or bf16 = the bf16 activation path); if its kernel produced per-block moment partials,
    finishes them into the stats record.  Returns stats [B, NSTAT] or None (caller then runs instnorm_stats)."""
    import ctypes
    lib = _lib.load()
    ws = workspace(int(lib.lg_conv_stats_workspace_bytes(int(up), B, Hs, Ws, cb if up else cs)), out.device, "statpart")
    nparts = ctypes.c_int(0)
    o16 = out.dtype == torch.bfloat16
    e0 = _pb()
    if x16 is not None:
        _chk16(x16, x if x is not None else x16, "x16")
    check(getattr(lib, fn_name)(_p(x), _p(x16), _p(pack), _p(bias), 0 if o16 else _p(out), _p(out) if o16 else 0, B, Hs, Ws, cb,
                                cs, dtype, _p(ws), ws.numel(), ctypes.addressof(nparts), _stream()), fn_name)
    _pe(e0, tag, flops)
    if nparts.value <= 0:
        return None
    if defer:   # the consumer (instnorm_apply) finishes the records in its own launch
        return Moments(ws, nparts.value, gamma, beta, B)
    stats = torch.empty(B, NSTAT, dtype=torch.float32, device=out.device)
    check(lib.lg_instnorm_stats_finalize(_p(ws), nparts.value, _p(stats), _p(gamma), _p(beta), B, _stream()),
          "lg_instnorm_stats_finalize")
    return stats


_FUSED_OK = {}


def _fwd_stats_z16(fn_name, x, x16, pack, bias, shape, B, Hs, Ws, cb, cs, dtype, gamma, beta, tag, flops, up, alpha, defer=False):
    """bf16 activation path: z leaves the conv as bf16.  Where the conv kernel fuses the moments (from its fp32
    accumulators) that is the only copy ever written; otherwise the conv writes fp32 once, the statistics pass reads it
    and emits the bf16 copy in the same sweep, and the fp32 tensor is dropped.  Either way:
    moments of the fp32 z, everything downstream reads bf16(z)."""
    dev = bias.device
    key = (int(up), dtype, B, Hs, Ws, cb, cs)
    if key not in _FUSED_OK:
        _FUSED_OK[key] = bool(_lib.load().lg_conv_fwd_stats_fused(*key))
    if _FUSED_OK[key]:
        z16 = torch.empty(shape, dtype=torch.bfloat16, device=dev)
        st = _fwd_stats(fn_name, x, x16, pack, bias, z16, B, Hs, Ws, cb, cs, dtype, gamma, beta, tag, flops, up, defer=defer)
        if st is None:
            raise _lib.LittleGanHipError(f"{fn_name}: lg_conv_fwd_stats_fused promised fused moments for {key}, none came")
        return z16, st
    z = torch.empty(shape, dtype=torch.float32, device=dev)
    st = _fwd_stats(fn_name, x, x16, pack, bias, z, B, Hs, Ws, cb, cs, dtype, gamma, beta, tag, flops, up)
    if st is not None:  # (moments fused although not promised: keep them, cast once)
        return z.to(torch.bfloat16), st
    z16 = torch.empty(shape, dtype=torch.bfloat16, device=dev)
    st = instnorm_stats(z, gamma, beta, 0, alpha, x16_out=z16)
    return z16, st


def conv2d_s2_fwd_stats(x, pack, bias, cs, dtype, gamma, beta, x16=None, z16=False, alpha=0.3, defer_stats=False):
    """conv2d_s2_fwd + the InstanceNormalization statistics of its output -> (z, stats or None).
    z16=True (bf16 dtype): z is returned as a bf16 tensor and stats is never None (see _fwd_stats_z16).
    defer_stats (with z16): where the conv fuses the moments, `stats` comes back as an unfinished ops.Moments for the next
    instnorm_apply to finish in its own launch (ops.stats_tensor() for any other use)."""
    B, H, W, cb = (x if x is not None else x16).shape  # x may be None when the bf16 mirror feeds the halo kernel
    if x is not None:
        _chk(x, name="x")
    _chk(bias, (cs,), "bias")
    if H % 2 or W % 2:
        raise ValueError("conv2d_s2_fwd_stats: H and W must be even")
    tag, fl = "conv_igemm_patch" if cb == 3 else "conv_igemm_down", 50.0 * B * (H // 2) * (W // 2) * cb * cs
    if z16:
        return _fwd_stats_z16("lg_conv2d_s2_fwd_stats", x, x16, pack, bias, (B, H // 2, W // 2, cs), B, H // 2, W // 2, cb, cs,
                              dtype, gamma, beta, tag, fl, False, alpha, defer=defer_stats)
    out = torch.empty(B, H // 2, W // 2, cs, dtype=torch.float32, device=bias.device)
    st = _fwd_stats("lg_conv2d_s2_fwd_stats", x, x16, pack, bias, out, B, H // 2, W // 2, cb, cs, dtype, gamma, beta, tag, fl,
                    up=False)
    return out, st


_ZN_OK = {}


def conv2d_s2_fwd_stats_zn_supported(B, H, W, cb, cs, dtype):
    """H x W: the map the conv reads (as conv2d_s2_fwd_stats).  True where conv2d_s2_fwd_stats_zn runs."""
    key = (B, H // 2, W // 2, cb, cs, dtype)
    if key not in _ZN_OK:
        _ZN_OK[key] = H % 2 == 0 and W % 2 == 0 and bool(_lib.load().lg_conv2d_s2_fwd_stats_zn_supported(*key))
    return _ZN_OK[key]


def conv2d_s2_fwd_stats_zn(zin16, zin_stats, alpha, pack, bias, cs, dtype, gamma, beta):
    """conv2d_s2_fwd_stats (bf16 path) fed with the RAW bf16 output zin16 [B,H,W,cb] of the level below and its statistics
    records: InstanceNorm + LeakyReLU(alpha) happen while the conv stages its operand, the normalised map is never written
    (bit-identical to instnorm_apply + conv2d_s2_fwd_stats).  -> (z16 [B,H/2,W/2,cs] bf16, stats [B, NSTAT])."""
    import ctypes
    lib = _lib.load()
    B, H, W, cb = zin16.shape
    _chk16(zin16, zin16, "zin16")
    _chk(zin_stats, (B, NSTAT), "zin_stats")
    _chk(bias, (cs,), "bias")
    if not conv2d_s2_fwd_stats_zn_supported(B, H, W, cb, cs, dtype):
        raise ValueError(f"conv2d_s2_fwd_stats_zn: shape {tuple(zin16.shape)} -> {cs} is outside the normalising kernel's tiling")
    Hs, Ws = H // 2, W // 2
    ws = workspace(int(lib.lg_conv_stats_workspace_bytes(0, B, Hs, Ws, cs)), zin16.device, "statpart")
    z16 = torch.empty(B, Hs, Ws, cs, dtype=torch.bfloat16, device=zin16.device)
    nparts = ctypes.c_int(0)
    e0 = _pb()
    check(lib.lg_conv2d_s2_fwd_stats_zn(_p(zin16), _p(zin_stats), float(alpha), _p(pack), _p(bias), _p(z16), B, Hs, Ws, cb, cs, dtype,
                                        _p(ws), ws.numel(), ctypes.addressof(nparts), _stream()), "lg_conv2d_s2_fwd_stats_zn")
    _pe(e0, "conv_igemm_down", 50.0 * B * Hs * Ws * cb * cs)
    if nparts.value <= 0:
        raise _lib.LittleGanHipError("lg_conv2d_s2_fwd_stats_zn: no moment partials came back")
    stats = torch.empty(B, NSTAT, dtype=torch.float32, device=zin16.device)
    check(lib.lg_instnorm_stats_finalize(_p(ws), nparts.value, _p(stats), _p(gamma), _p(beta), B, _stream()),
          "lg_instnorm_stats_finalize")
    return z16, stats


def convT_s2_fwd_stats(x, pack, bias, cb, dtype, gamma, beta, x16=None, z16=False, alpha=0.3, defer_stats=False):
    B, Hs, Ws, cs = (x if x is not None else x16).shape
    if x is not None:
        _chk(x, name="x")
    _chk(bias, (cb,), "bias")
    fl = 50.0 * B * Hs * Ws * cb * cs
    if z16:
        return _fwd_stats_z16("lg_convT_s2_fwd_stats", x, x16, pack, bias, (B, 2 * Hs, 2 * Ws, cb), B, Hs, Ws, cb, cs, dtype,
                              gamma, beta, "conv_igemm_up", fl, True, alpha, defer=defer_stats)
    out = torch.empty(B, 2 * Hs, 2 * Ws, cb, dtype=torch.float32, device=bias.device)
    st = _fwd_stats("lg_convT_s2_fwd_stats", x, x16, pack, bias, out, B, Hs, Ws, cb, cs, dtype, gamma, beta, "conv_igemm_up", fl,
                    up=True)
    return out, st


_NS_OK = {}


def convT_s2_fwd_ns_supported(B, Hs, Ws, cb, cs, dtype):
    """Hs x Ws: the map the transposed conv reads (as convT_s2_fwd_stats).  True where convT_s2_fwd_stats_ns runs."""
    key = (B, Hs, Ws, cb, cs, dtype)
    if key not in _NS_OK:
        _NS_OK[key] = bool(_lib.load().lgadj_convT_s2_fwd_ns_supported(*key))
    return _NS_OK[key]


_GRID_CUS = []


def _fills_the_grid(B, Hm, Wm):
    """B maps of Hm x Wm tile origins (8 x 16 tiles of conv_up3 / conv_down3) give every CU's persistent workgroup at least one tile"""
    if not _GRID_CUS:
        _GRID_CUS.append(int(_lib.load().lg_grid_cus()))
    return B * (Hm // 8) * (Wm // 16) >= max(_GRID_CUS[0], 1)


# Adoption of the Adjuster's fused routes ("Adoption").  Each route trades apply launches for ONE stand-alone finalize
# launch (~5 us) in front of the consuming conv: the decoder's two apply launches of a level, the encoder's one.  It pays where the
# apply passes are HBM-bound, which is where it was measured (2B = 512, B = 256: every level wins).  A batch that does not even give
# every CU one tile of the consuming conv is launch-bound: an apply launch there costs what the finalize launch costs, the encoder's
# trade is one launch for one launch, and nothing was measured — such a batch stays on the apply route.
def convT_s2_fwd_ns_adopted(B, Hs, Ws, cb, cs, dtype):
    """Hs x Ws: the map the transposed conv reads.  True where the Adjuster's decoder leaves norm + skip to convT_s2_fwd_stats_ns."""
    return convT_s2_fwd_ns_supported(B, Hs, Ws, cb, cs, dtype) and _fills_the_grid(B, Hs, Ws)


def enc_raw_skip_adopted(B, H, W, cb, cs, dtype):
    """H x W: the map the conv reads (as conv2d_s2_fwd_stats_zn_supported).  True where the Adjuster's own encoder pass hands that
    map over un-normalised and feeds the conv through conv2d_s2_fwd_stats_zn."""
    return conv2d_s2_fwd_stats_zn_supported(B, H, W, cb, cs, dtype) and _fills_the_grid(B, H // 2, W // 2)


def convT_s2_fwd_stats_ns(zin16, zin_stats, alpha, skip, pack, bias, cb, dtype, gamma, beta, defer_stats=False):
    """convT_s2_fwd_stats (bf16 path) of the input h = bf16(LeakyReLU(InstanceNorm(zin16)) + skip), formed while the kernel stages its
    operand: h is never written (bit-identical to instnorm_apply with that skip + convT_s2_fwd_stats).  zin16 [B,Hs,Ws,cs]: the raw
    bf16 output of the level below, zin_stats its FINISHED records.  skip: a bf16 map or an ops.Raw of zin16's shape, or a pair of them
    (first rows, remaining rows) of the batch.  -> (z16 [B,2Hs,2Ws,cb] bf16, stats: [B, NSTAT], or unfinished Moments if defer_stats)."""
    import ctypes
    lib = _lib.load()
    B, Hs, Ws, cs = zin16.shape
    _chk16(zin16, zin16, "zin16")
    _chk(zin_stats, (B, NSTAT), "zin_stats")
    _chk(bias, (cb,), "bias")
    if not convT_s2_fwd_ns_supported(B, Hs, Ws, cb, cs, dtype):
        raise ValueError(f"convT_s2_fwd_stats_ns: shape {tuple(zin16.shape)} -> {cb} is outside the normalising kernel's tiling")
    parts = skip if isinstance(skip, tuple) else (skip, None)
    b1 = parts[0].shape[0] if parts[0] is not None else 0
    if not 0 <= b1 <= B or (b1 < B and parts[1] is None):
        raise ValueError("convT_s2_fwd_stats_ns: the skip parts do not cover the batch")
    args = []
    for part, rows in zip(parts, (b1, B - b1)):
        if part is None or rows == 0:
            args += [0, 0]
            continue
        z = part.z if isinstance(part, Raw) else part
        if tuple(z.shape) != (rows, Hs, Ws, cs):
            raise ValueError(f"convT_s2_fwd_stats_ns: a skip part has shape {tuple(z.shape)}, expected {(rows, Hs, Ws, cs)}")
        _chk16(z, z, "skip")
        args += [_p(z), _p(part.stats) if isinstance(part, Raw) else 0]
    ws = workspace(int(lib.lg_conv_stats_workspace_bytes(1, B, Hs, Ws, cb)), zin16.device, "statpart")
    z16 = torch.empty(B, 2 * Hs, 2 * Ws, cb, dtype=torch.bfloat16, device=zin16.device)
    nparts = ctypes.c_int(0)
    e0 = _pb()
    check(lib.lgadj_convT_s2_fwd_stats_ns(_p(zin16), _p(zin_stats), float(alpha), *args, b1, _p(pack), _p(bias), _p(z16), B, Hs, Ws, cb,
                                          cs, dtype, _p(ws), ws.numel(), ctypes.addressof(nparts), _stream()),
          "lgadj_convT_s2_fwd_stats_ns")
    _pe(e0, "conv_igemm_up", 50.0 * B * Hs * Ws * cb * cs)
    if nparts.value <= 0:
        raise _lib.LittleGanHipError("lgadj_convT_s2_fwd_stats_ns: no moment partials came back")
    if defer_stats:
        return z16, Moments(ws, nparts.value, gamma, beta, B)
    stats = torch.empty(B, NSTAT, dtype=torch.float32, device=zin16.device)
    check(lib.lg_instnorm_stats_finalize(_p(ws), nparts.value, _p(stats), _p(gamma), _p(beta), B, _stream()),
          "lg_instnorm_stats_finalize")
    return z16, stats


# ------------------------------------------------------------------ step inputs on the device (eager_trainer.py:125-131)
def _i64(v):
    """unsigned 64-bit value as the signed pattern ctypes' c_longlong takes"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def philox4x32(nblocks, seed, offset, device="cuda"):
    out = torch.empty(nblocks * 4, dtype=torch.int32, device=device)
    check(_lib.load().lg_philox4x32(_p(out), nblocks, _i64(seed), _i64(offset), _stream()), "lg_philox4x32")
    return out


def randn(shape, seed, offset, mean=0.0, std=1.0, device="cuda"):
    """tf.random.normal(shape, mean, std) from the counter-based generator: reproducible per (seed, offset)."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(_lib.load().lg_randn(_p(out), out.numel(), float(mean), float(std), _i64(seed), _i64(offset), _stream()), "lg_randn")
    return out


def augment(img, flip, db, cf, dh, noise_scale, seed, offset, out=None):
    """flip: uint8 [B] device tensor or None; see lg_augment."""
    B, H, W, c = img.shape
    _chk(img, name="img")
    if c != 3:
        raise ValueError("augment: 3-channel images only")
    if out is None:
        out = torch.empty_like(img)
    _chk(out, img.shape, "out")
    if flip is not None and not (flip.is_cuda and flip.dtype == torch.uint8 and flip.numel() == B and flip.is_contiguous()):
        raise ValueError("augment: flip must be a contiguous uint8 CUDA tensor with B elements")
    lib = _lib.load()
    ws = workspace(int(lib.lg_augment_workspace_bytes(B)), img.device, "small")
    check(lib.lg_augment(_p(img), _p(out), B, H, W, _p(flip), float(db), float(cf), float(dh), float(noise_scale),
                         _i64(seed), _i64(offset), _p(ws), ws.numel(), _stream()), "lg_augment")
    return out


def augment_drawn(img, db_max, c_lo, c_hi, dh_max, noise_scale, seed, draw_offset, noise_offset, out=None):
    """lg_augment_drawn: flip / brightness / contrast / hue draws made on the device from the Philox window at
    draw_offset (no host synchronisation); see include/littlegan_hip.h."""
    B, H, W, c = img.shape
    _chk(img, name="img")
    if c != 3:
        raise ValueError("augment_drawn: 3-channel images only")
    if out is None:
        out = torch.empty_like(img)
    _chk(out, img.shape, "out")
    lib = _lib.load()
    ws = workspace(int(lib.lg_augment_drawn_workspace_bytes(B)), img.device, "small")
    check(lib.lg_augment_drawn(_p(img), _p(out), B, H, W, float(db_max), float(c_lo), float(c_hi), float(dh_max),
                               float(noise_scale), _i64(seed), _i64(draw_offset), _i64(noise_offset), _p(ws), ws.numel(),
                               _stream()), "lg_augment_drawn")
    return out


# ------------------------------------------------------------------ differentiable augmentation of D's inputs (diffaug.hip)
def _chk_key(key, what):
    if not (isinstance(key, torch.Tensor) and key.is_cuda and key.dtype == torch.int64 and key.numel() == 2 and key.is_contiguous()):
        raise ValueError(f"{what}: key must be a contiguous int64 CUDA tensor {{seed, key_offset}}")


def diffaug_draw(key, call, r0, rows, S, policy, out=None):
    """params [rows, 8] fp32 = the records {b, s, c, ty, tx, cy, cx, cut} of rows r0 .. r0+rows-1 of call slot `call` under the step's
    key (int64 [2] device tensor {seed, key_offset}: dropout_key writes such a pair); policy: the diff_augment string or its bits."""
    from .config import diff_augment_bits
    bits = int(policy) if isinstance(policy, int) else diff_augment_bits(policy)
    _chk_key(key, "diffaug_draw")
    if out is None:
        out = torch.empty(int(rows), 8, dtype=torch.float32, device=key.device)
    _chk(out, (int(rows), 8), "out")
    check(_lib.load().lg_diffaug_draw(_p(key), int(call), int(r0), int(rows), int(S), bits, _p(out), _stream()), "lg_diffaug_draw")
    return out


def _diffaug_map(fn_name, v, params, out):
    _chk(v, name="image")
    rows, S, W, c = v.shape
    if W != S or c != 3:
        raise ValueError(f"{fn_name}: square 3-channel NHWC images only, got {tuple(v.shape)}")
    _chk(params, (rows, 8), "params")
    if out is None:
        out = torch.empty_like(v)
    _chk(out, v.shape, "out")
    lib = _lib.load()
    ws = workspace(int(lib.lg_diffaug_workspace_bytes(rows, S)), v.device, "small")
    check(getattr(lib, fn_name)(_p(v), _p(params), _p(out), rows, S, _p(ws), ws.numel(), _stream()), fn_name)
    return out


def diffaug_fwd(x, params, out=None):
    """T(x): x [rows, S, S, 3] fp32 under params [rows, 8] (diffaug_draw, or hand-built records); see include/littlegan_hip.h"""
    return _diffaug_map("lg_diffaug_fwd", x, params, out)


def diffaug_bwd(g, params, out=None):
    """The exact adjoint of diffaug_fwd: the gradient w.r.t. x of <T(x), g>"""
    return _diffaug_map("lg_diffaug_bwd", g, params, out)


# ------------------------------------------------------------------ adaptive augmentation probability (ada.hip)
def _chk_ada(state, what):
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.float32 and state.numel() == 4
            and state.is_contiguous()):
        raise ValueError(f"{what}: state must be a contiguous fp32 CUDA tensor of 4 words {{p, sum, rows, steps}} (ada_init)")


def diffaug_draw_gated(key, call, r0, rows, S, policy, state, out=None):
    """diffaug_draw with each named component of each row applied with probability p = state[0] (read on the device): a component that
    is gated off gets its identity values.  p = 1 is diffaug_draw bit for bit.  See include/littlegan_hip_ext.h"""
    from .config import diff_augment_bits
    bits = int(policy) if isinstance(policy, int) else diff_augment_bits(policy)
    _chk_key(key, "diffaug_draw_gated")
    _chk_ada(state, "diffaug_draw_gated")
    if out is None:
        out = torch.empty(int(rows), 8, dtype=torch.float32, device=key.device)
    _chk(out, (int(rows), 8), "out")
    check(_lib.load().lgx_diffaug_draw_gated(_p(key), int(call), int(r0), int(rows), int(S), bits, _p(state), _p(out), _stream()),
          "lgx_diffaug_draw_gated")
    return out


def ada_init(p0, device="cuda", out=None):
    """The controller's state {p0, 0, 0, 0} (fp32 [4]: fp32 p, then the int32 sum of signs, rows and steps of the interval), written by a
    one-block kernel from a launch scalar: no host-to-device copy."""
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=device)
    _chk_ada(out, "ada_init")
    check(_lib.load().lgx_ada_init(_p(out), float(p0), _stream()), "lgx_ada_init")
    return out


def ada_accumulate(state, heads, B):
    """One step's statistic: sum += sum_i sign(heads[i, 0] - 0.5) over the first B rows of D's packed output [rows, 1 + c]; rows += B;
    steps += 1"""
    _chk_ada(state, "ada_accumulate")
    _chk(heads, name="heads")
    if heads.dim() != 2 or not 1 <= int(B) <= heads.shape[0]:
        raise ValueError(f"ada_accumulate: heads must be [rows >= B, 1 + c], got {tuple(heads.shape)} with B = {B}")
    check(_lib.load().lgx_ada_accumulate(_p(state), _p(heads), heads.shape[1], int(B), _stream()), "lgx_ada_accumulate")
    return state


def ada_adjust(state, interval, target, per_row):
    """The controller: once `interval` steps are in, p moves by rows * per_row towards sum / rows == target, is clamped to [0, 1], and
    the counters restart; before that nothing is written."""
    _chk_ada(state, "ada_adjust")
    check(_lib.load().lgx_ada_adjust(_p(state), int(interval), float(target), float(per_row), _stream()), "lgx_ada_adjust")
    return state


def ada_read(state):
    """(p, sum, rows, steps) on the host.  Synchronises: for logs, checkpoints and tests, not for the step."""
    _chk_ada(state, "ada_read")
    host = state.detach().cpu()
    w = host.view(torch.int32).tolist()
    return float(host[0]), w[1], w[2], w[3]


# ------------------------------------------------------------------ geometric augmentation of D's inputs (geom.hip)
def geom_draw(key, call, r0, rows, S, policy, state=None, out=None):
    """geo [rows, 4] fp32 = the records {a, b, c, d} (M = R(theta) Q^k F / s, destination -> source about the centre) of rows
    r0 .. r0+rows-1 of call slot `call` under the step's diff_augment key; policy: the geom_augment string or its bits; state: None =
    every named component on every row, else the ADA state whose p gates each component per row.  See include/littlegan_geom.h"""
    from .config import geom_augment_bits
    bits = int(policy) if isinstance(policy, int) else geom_augment_bits(policy)
    _chk_key(key, "geom_draw")
    if state is not None:
        _chk_ada(state, "geom_draw")
    if out is None:
        out = torch.empty(int(rows), 4, dtype=torch.float32, device=key.device)
    _chk(out, (int(rows), 4), "out")
    check(_lib.load().lgeo_draw(_p(key), int(call), int(r0), int(rows), int(S), bits, None if state is None else _p(state), _p(out),
                                _stream()), "lgeo_draw")
    return out


def _geom_map(fn_name, v, geo, out):
    _chk(v, name="image")
    rows, S, W, c = v.shape
    if W != S or c != 3:
        raise ValueError(f"{fn_name}: square 3-channel NHWC images only, got {tuple(v.shape)}")
    _chk(geo, (rows, 4), "geo")
    if out is None:
        out = torch.empty_like(v)
    _chk(out, v.shape, "out")
    check(getattr(_lib.load(), fn_name)(_p(v), _p(geo), _p(out), rows, S, _stream()), fn_name)
    return out


def geom_fwd(x, geo, out=None):
    """Geo(x): x [rows, S, S, 3] fp32 resampled bilinearly (zero fill) under geo [rows, 4] (geom_draw, or hand-built records)"""
    return _geom_map("lgeo_fwd", x, geo, out)


def geom_bwd(g, geo, out=None):
    """The exact adjoint of geom_fwd: the gradient w.r.t. x of <Geo(x), g>, gathered in a fixed order"""
    return _geom_map("lgeo_bwd", g, geo, out)



# ------------------------------------------------------------------ packed uint8 data set (input_u8.hip)
def _chk_rows(src, idx, name):
    """src: contiguous uint8 CUDA tensor [N, ...]; idx: contiguous int64 CUDA vector of row numbers (the kernels trust them)"""
    if not (src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() >= 2):
        raise ValueError(f"{name}: src must be a contiguous uint8 CUDA tensor [N, ...], got {src.dtype} {src.device}")
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 1 and idx.numel() > 0):
        raise ValueError(f"{name}: idx must be a non-empty contiguous int64 CUDA vector, got {idx.dtype} {idx.device}")


def rescale_u8(src, idx, out=None):
    """lg_rescale_u8: out[b] = data_rescale(src[idx[b]]) as float32, shape [B, *src.shape[1:]]."""
    _chk_rows(src, idx, "rescale_u8")
    B, row = idx.numel(), src[0].numel()
    if out is None:
        out = torch.empty((B,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    _chk(out, (B,) + tuple(src.shape[1:]), "out")
    check(_lib.load().lg_rescale_u8(_p(src), _p(idx), B, row, _p(out), _stream()), "lg_rescale_u8")
    return out


def soft_labels(attr, idx, cols, out=None):
    """lg_soft_labels: out[b][j] = soft(attr[idx[b]][cols[j]]); attr fp32 [N, A_all], cols int32 [c], both on the device."""
    _chk(attr, name="attr")
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 1 and idx.numel() > 0):
        raise ValueError("soft_labels: idx must be a non-empty contiguous int64 CUDA vector")
    if not (cols.is_cuda and cols.dtype == torch.int32 and cols.is_contiguous() and cols.dim() == 1 and cols.numel() > 0):
        raise ValueError("soft_labels: cols must be a non-empty contiguous int32 CUDA vector")
    B, c = idx.numel(), cols.numel()
    if out is None:
        out = torch.empty((B, c), dtype=torch.float32, device=attr.device)
    _chk(out, (B, c), "out")
    check(_lib.load().lg_soft_labels(_p(attr), _p(idx), _p(cols), B, attr.shape[1], c, _p(out), _stream()), "lg_soft_labels")
    return out


def augment_drawn_u8(src, idx, db_max, c_lo, c_hi, dh_max, noise_scale, seed, draw_offset, noise_offset, out=None,
                     out_rescaled=None, want_rescaled=True):
    """lg_augment_drawn_u8: (augment_drawn(rescale_u8(src, idx)), rescale_u8(src, idx)) from one read of the bytes; the
    second is None when want_rescaled is false.  src uint8 [N, H, W, 3]."""
    _chk_rows(src, idx, "augment_drawn_u8")
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError("augment_drawn_u8: 3-channel [N, H, W, 3] images only")
    B, (H, W) = idx.numel(), src.shape[1:3]
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.float32, device=src.device)
    _chk(out, (B, H, W, 3), "out")
    if want_rescaled and out_rescaled is None:
        out_rescaled = torch.empty((B, H, W, 3), dtype=torch.float32, device=src.device)
    if out_rescaled is not None:
        _chk(out_rescaled, (B, H, W, 3), "out_rescaled")
    lib = _lib.load()
    ws = workspace(int(lib.lg_augment_drawn_u8_workspace_bytes(B)), src.device, "small")
    check(lib.lg_augment_drawn_u8(_p(src), _p(idx), _p(out), _p(out_rescaled), B, H, W, float(db_max), float(c_lo), float(c_hi),
                                  float(dh_max), float(noise_scale), _i64(seed), _i64(draw_offset), _i64(noise_offset), _p(ws),
                                  ws.numel(), _stream()), "lg_augment_drawn_u8")
    return out, out_rescaled


def fid_stats(act):
    """fid.py:185-188 on the device: (mu [D], sigma [D, D]) fp64 tensors of act [N, D] (fp32 CUDA)."""
    if act.dim() != 2 or act.shape[0] < 2:
        raise ValueError("fid_stats: need an [N >= 2, D] matrix")
    _chk(act, name="act")
    N, D = act.shape
    mu = torch.empty(D, dtype=torch.float64, device=act.device)
    sigma = torch.empty(D, D, dtype=torch.float64, device=act.device)
    lib = _lib.load()
    ws = workspace(int(lib.lg_fid_stats_workspace_bytes(N, D)), act.device, "small")
    check(lib.lg_fid_stats(_p(act), N, D, _p(mu), _p(sigma), _p(ws), ws.numel(), _stream()), "lg_fid_stats")
    return mu, sigma


def fid_gram_elems(D):
    """doubles in the packed upper-triangular 64 x 64 tile image of a D x D Gram matrix (lg_fid_accum)"""
    nt = (int(D) + 63) // 64
    return nt * (nt + 1) // 2 * 4096


def _chk64(t, shape, name):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: need a contiguous fp64 CUDA tensor of shape {tuple(shape)}, got {t.dtype} {t.device} {tuple(t.shape)}")
    return t


def fid_accum(act, sum, gram, shift=None):
    """fid.py:185-188 batch by batch: sum [D] += S (x - shift), gram [fid_gram_elems(D)] += S (x - shift)(x - shift)^T (packed
    upper-triangular tiles) over the rows of act [n >= 1, D] (fp32 CUDA).  sum / gram: fp64, zero before the first batch."""
    if act.dim() != 2 or act.shape[0] < 1:
        raise ValueError("fid_accum: need an [n >= 1, D] matrix")
    _chk(act, name="act")
    n, D = act.shape
    _chk64(sum, (D,), "sum")
    _chk64(gram, (fid_gram_elems(D),), "gram")
    if shift is not None:
        _chk64(shift, (D,), "shift")
    check(_lib.load().lg_fid_accum(_p(act), n, D, _p(shift), _p(sum), _p(gram), _stream()), "lg_fid_accum")


def fid_finalize(sum, gram, count, shift=None):
    """(mu [D], sigma [D, D]) fp64 from the accumulated state of `count` >= 2 samples; sigma is exactly symmetric."""
    if sum.dim() != 1 or int(count) < 2:
        raise ValueError("fid_finalize: need a [D] sum and at least 2 samples")
    D = sum.shape[0]
    _chk64(sum, (D,), "sum")
    _chk64(gram, (fid_gram_elems(D),), "gram")
    if shift is not None:
        _chk64(shift, (D,), "shift")
    mu = torch.empty(D, dtype=torch.float64, device=sum.device)
    sigma = torch.empty(D, D, dtype=torch.float64, device=sum.device)
    check(_lib.load().lg_fid_finalize(_p(sum), _p(gram), _p(shift), int(count), D, _p(mu), _p(sigma), _stream()), "lg_fid_finalize")
    return mu, sigma


def fid_gemm(a, b, alpha=1.0, beta=0.0):
    """alpha a b + beta I of two [D, D] fp64 CUDA matrices on the fp64 matrix instruction (the GEMM of lg_fid_distance; tests, bench)."""
    if a.dim() != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("fid_gemm: need square matrices")
    D = a.shape[0]
    _chk64(a, (D, D), "a")
    _chk64(b, (D, D), "b")
    import ctypes
    c = torch.empty_like(a)
    ab = (ctypes.c_double * 2)(float(alpha), float(beta))
    check(_lib.load().lg_fid_gemm(_p(a), _p(b), _p(c), D, ctypes.addressof(ab), _stream()), "lg_fid_gemm")
    return c


def fid_distance(mu1, s1, mu2, s2, max_iter=100):
    """Frechet distance (fid.py:112-163) with tr sqrt(S1 S2) by the coupled Newton-Schulz iteration on the device, fp64.
    -> (d2, tr_sqrt, iterations, status); status 1 = not converged.  Synchronises the stream; not capturable in a graph."""
    if mu1.dim() != 1 or int(max_iter) < 1:
        raise ValueError("fid_distance: need [D] means and max_iter >= 1")
    D = mu1.shape[0]
    _chk64(mu1, (D,), "mu1")
    _chk64(mu2, (D,), "mu2")
    _chk64(s1, (D, D), "sigma1")
    _chk64(s2, (D, D), "sigma2")
    import ctypes
    lib = _lib.load()
    ws = workspace(int(lib.lg_fid_distance_workspace_bytes(D)), mu1.device, "fid_sqrt")
    res = (ctypes.c_double * 4)()
    check(lib.lg_fid_distance(_p(mu1), _p(s1), _p(mu2), _p(s2), D, int(max_iter), ctypes.addressof(res), _p(ws), ws.numel(), _stream()),
          "lg_fid_distance")
    return float(res[0]), float(res[1]), int(res[2]), int(res[3])


# ------------------------------------------------------------------ pairwise passes of the sample metrics (pairs.hip)
def _chk_pair(x, y, who):
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] < 1 or y.shape[0] < 1 or x.shape[1] < 1 or x.shape[1] != y.shape[1]:
        raise ValueError(f"{who}: need [n >= 1, D] and [m >= 1, D] matrices with the same D >= 1, got {tuple(x.shape)} and {tuple(y.shape)}")
    _chk(x, name="x")
    _chk(y, name="y")
    return x.shape[0], y.shape[0], x.shape[1]


def pairs_workspace_bytes(n, m, D):
    return int(_lib.load().lg_pairs_workspace_bytes(int(n), int(m), int(D)))


def pairs_poly_sum(x, y, sums, degree=3, gamma=None, coef0=1.0, diag=False):
    """sums [2] (fp64 CUDA) += (sum_ij k_ij, sum_i k_ii when diag) with k_ij = (gamma x_i . y_j + coef0)^degree over x [n, D] against
    y [m, D] (fp32 CUDA); gamma None = 1 / D.  diag says that x and y are the same rows.  Bit-reproducible."""
    n, m, D = _chk_pair(x, y, "pairs_poly_sum")
    if not 1 <= int(degree) <= 8:
        raise ValueError(f"pairs_poly_sum: degree {degree} outside 1..8")
    if diag and n != m:
        raise ValueError(f"pairs_poly_sum: diag needs the same rows on both sides, got n={n} m={m}")
    _chk64(sums, (2,), "sums")
    import ctypes
    lib = _lib.load()
    gc = (ctypes.c_double * 2)(1.0 / D if gamma is None else float(gamma), float(coef0))
    ws = workspace(int(lib.lg_pairs_workspace_bytes(n, m, D)), x.device, "pairs")
    check(lib.lg_pairs_poly_sum(_p(x), n, _p(y), m, D, int(degree), ctypes.addressof(gc), int(bool(diag)), _p(sums), _p(ws), ws.numel(),
                                _stream()), "lg_pairs_poly_sum")
    return sums


def pairs_knn(x, y, best):
    """best [n, kk] (fp64 CUDA, ascending, +inf before the first call) <- the kk smallest squared distances of every row of x [n, D]
    over its present entries and the rows of y [m, D] (fp32 CUDA).  1 <= kk <= 16."""
    n, m, D = _chk_pair(x, y, "pairs_knn")
    if best.dim() != 2 or not 1 <= best.shape[1] <= 16:
        raise ValueError(f"pairs_knn: best must be [n, 1 <= kk <= 16], got {tuple(best.shape)}")
    _chk64(best, (n, best.shape[1]), "best")
    lib = _lib.load()
    ws = workspace(int(lib.lg_pairs_workspace_bytes(n, m, D)), x.device, "pairs")
    check(lib.lg_pairs_knn(_p(x), n, _p(y), m, D, int(best.shape[1]), _p(best), _p(ws), ws.numel(), _stream()), "lg_pairs_knn")
    return best


def pairs_ball_count(q, ref, radius2, count):
    """count [n] (int32 CUDA) += #{ j : |q_i - ref_j|^2 <= radius2[j] } over q [n, D] against ref [m, D] (fp32 CUDA), radius2 [m] fp64."""
    n, m, D = _chk_pair(q, ref, "pairs_ball_count")
    _chk64(radius2, (m,), "radius2")
    if not (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous()) or tuple(count.shape) != (n,):
        raise ValueError(f"count: need a contiguous int32 CUDA tensor of shape ({n},), got {count.dtype} {count.device} {tuple(count.shape)}")
    lib = _lib.load()
    ws = workspace(int(lib.lg_pairs_workspace_bytes(n, m, D)), q.device, "pairs")
    check(lib.lg_pairs_ball_count(_p(q), n, _p(ref), m, _p(radius2), D, _p(count), _p(ws), ws.numel(), _stream()), "lg_pairs_ball_count")
    return count


# ------------------------------------------------------------------ discriminator gradient penalty (gp.hip)
def gp_draw_eps(B, seed, offset, device="cuda"):
    """eps [B] ~ U[0, 1) from the counter-based generator (lg_gp_draw_eps): the interpolation weights of the penalty."""
    out = torch.empty(B, dtype=torch.float32, device=device)
    check(_lib.load().lg_gp_draw_eps(_p(out), int(B), _i64(seed), _i64(offset), _stream()), "lg_gp_draw_eps")
    return out


def gp_interp(real, fake, eps, out=None):
    """x^ = eps_b real_b + (1 - eps_b) fake_b"""
    _chk(real, name="real")
    _chk(fake, real.shape, "fake")
    B = real.shape[0]
    _chk(eps, (B,), "eps")
    if out is None:
        out = torch.empty_like(real)
    _chk(out, real.shape, "out")
    check(_lib.load().lg_gp_interp(_p(real), _p(fake), _p(eps), _p(out), B, real.numel() // B, _stream()), "lg_gp_interp")
    return out


def _gp_ws(B, L, device):
    return workspace(int(_lib.load().lg_gp_workspace_bytes(B, L)), device, "gp")


def gp_seed(g, gp_weight, loss=None, gp_loss=None):
    """g = the image gradient of p: -> (u0 = d(gp_weight gp)/dg, r [B]); loss (+)= gp_weight gp, gp_loss = gp_weight gp"""
    _chk(g, name="g")
    B = g.shape[0]
    L = g.numel() // B
    for t, nm in ((loss, "loss"), (gp_loss, "gp_loss")):
        if t is not None:
            _chk(t, (1,), nm)
    u0 = torch.empty_like(g)
    r = torch.empty(B, dtype=torch.float32, device=g.device)
    ws = _gp_ws(B, L, g.device)
    check(_lib.load().lg_gp_seed(_p(g), _p(u0), _p(r), _p(loss), _p(gp_loss), float(gp_weight), _p(ws), ws.numel(), B, L,
                                 _stream()), "lg_gp_seed")
    return u0, r


def _gp_z(z, g, stats, gamma):
    B = z.shape[0]
    if z.dtype == torch.bfloat16:
        _chk16(z, z, "z")
    else:
        _chk(z, name="z")
    _chk(g, z.shape, "g")
    _chk(stats, (B, NSTAT), "stats")
    _chk(gamma, (1,), "gamma")
    return (None, z) if z.dtype == torch.bfloat16 else (z, None)


def gp_norm_bwd(z, stats, gamma, g, alpha, add=None, dgamma=None, dbeta=None, out16=None, want_f32=True):
    """first-order InstanceNorm + LeakyReLU backward of a level (z: fp32 or its bf16 raw output) with an optional injected
    adjoint `add` on dz; dgamma / dbeta (+)= when given.  Returns dz (fp32, or None with want_f32=False: only out16)."""
    z32, z16 = _gp_z(z, g, stats, gamma)
    B = z.shape[0]
    L = z.numel() // B
    if add is not None:
        _chk(add, z.shape, "add")
    for t, nm in ((dgamma, "dgamma"), (dbeta, "dbeta")):
        if t is not None:
            _chk(t, (1,), nm)
    if out16 is not None:
        _chk16(out16, z, "out16")
    elif not want_f32:
        raise ValueError("gp_norm_bwd: want_f32=False needs out16")
    dz = torch.empty(z.shape, dtype=torch.float32, device=z.device) if want_f32 else None
    ws = _gp_ws(B, L, z.device)
    e0 = _pb()
    check(_lib.load().lg_gp_norm_bwd(_p(z32), _p(z16), _p(stats), _p(gamma), _p(g), _p(add), _p(dz), _p(out16), _p(dgamma),
                                     _p(dbeta), _p(ws), ws.numel(), B, L, float(alpha), _stream()), "lg_gp_norm_bwd")
    _pe(e0, "gp_norm", 0.0)
    return dz


def gp_norm_dd(z, stats, gamma, g, u, alpha, dgamma=None, want_uz2=True):
    """double backward of the level's InstanceNorm + LeakyReLU along the adjoint u of its dz -> (u_h, u_z2 | None)"""
    z32, z16 = _gp_z(z, g, stats, gamma)
    B = z.shape[0]
    L = z.numel() // B
    _chk(u, z.shape, "u")
    if dgamma is not None:
        _chk(dgamma, (1,), "dgamma")
    uh = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    uz2 = torch.empty(z.shape, dtype=torch.float32, device=z.device) if want_uz2 else None
    ws = _gp_ws(B, L, z.device)
    e0 = _pb()
    check(_lib.load().lg_gp_norm_dd(_p(z32), _p(z16), _p(stats), _p(gamma), _p(g), _p(u), _p(uh), _p(uz2), _p(dgamma), _p(ws),
                                    ws.numel(), B, L, float(alpha), _stream()), "lg_gp_norm_dd")
    _pe(e0, "gp_norm", 0.0)
    return uh, uz2


def gp_heads_seed(p, wpr):
    """g [B, K] = p_b (1 - p_b) wpr: the gradient of output_pr on the heads input"""
    _chk(p, name="p")
    B, J = p.shape
    K = wpr.shape[0]
    _chk(wpr, (K, 1), "wpr")
    g = torch.empty(B, K, dtype=torch.float32, device=p.device)
    check(_lib.load().lg_gp_heads_seed(_p(p), _p(wpr), _p(g), B, K, J - 1, _stream()), "lg_gp_heads_seed")
    return g


def gp_heads_2nd(p, wpr, x, u, dwpr=None, dbpr=None):
    """second order at the heads along the adjoint u [B, K] -> (t [B], g2 [B, K] = t_b wpr); dwpr / dbpr (+)= when given"""
    _chk(p, name="p")
    B, J = p.shape
    K = wpr.shape[0]
    _chk(wpr, (K, 1), "wpr")
    _chk(u, (B, K), "u")
    if x is not None:
        _chk(x, (B, K), "x")
    if dwpr is not None:
        _chk(dwpr, (K, 1), "dwpr")
        if x is None:
            raise ValueError("gp_heads_2nd: dwpr needs the heads input x")
    if dbpr is not None:
        _chk(dbpr, (1,), "dbpr")
    t = torch.empty(B, dtype=torch.float32, device=p.device)
    g2 = torch.empty(B, K, dtype=torch.float32, device=p.device)
    check(_lib.load().lg_gp_heads_2nd(_p(p), _p(wpr), _p(x), _p(u), _p(t), _p(g2), _p(dwpr), _p(dbpr), B, K, J - 1, _stream()),
          "lg_gp_heads_2nd")
    return t, g2


# ------------------------------------------------------------------ R1 gradient penalty (r1.hip; include/littlegan_hip_reg.h)
def r1_heads_seed(wpr, B):
    """g [B, K] = wpr for every row: the gradient of the pre-sigmoid output_pr on the heads input (step 2 of the pass)"""
    K = wpr.shape[0]
    _chk(wpr, (K, 1), "wpr")
    g = torch.empty(int(B), K, dtype=torch.float32, device=wpr.device)
    check(_lib.load().lgr_r1_heads_seed(_p(wpr), _p(g), int(B), K, _stream()), "lgr_r1_heads_seed")
    return g


def r1_seed(g, weight, loss=None, r1_loss=None):
    """g = the image gradient of the logit: -> (u0 = (weight / B) g, r2 [B] = |g_b|^2); loss (+)= term, r1_loss = term with
    term = (weight / 2) mean_b r2 (step 4)"""
    _chk(g, name="g")
    B = g.shape[0]
    L = g.numel() // B
    for t, nm in ((loss, "loss"), (r1_loss, "r1_loss")):
        if t is not None:
            _chk(t, (1,), nm)
    u0 = torch.empty_like(g)
    r2 = torch.empty(B, dtype=torch.float32, device=g.device)
    lib = _lib.load()
    ws = workspace(int(lib.lgr_r1_workspace_bytes(B, L)), g.device, "r1")
    check(lib.lgr_r1_seed(_p(g), _p(u0), _p(r2), _p(loss), _p(r1_loss), float(weight), _p(ws), ws.numel(), B, L, _stream()), "lgr_r1_seed")
    return u0, r2


def r1_heads_colsum(u, dwpr):
    """dwpr [K, 1] += sum_b u[b] (step 6: the logit is bilinear in (w_pr, h4), so this is all the heads receive)"""
    _chk(u, name="u")
    B, K = u.shape
    _chk(dwpr, (K, 1), "dwpr")
    lib = _lib.load()
    ws = workspace(int(lib.lgr_r1_colsum_workspace_bytes(B, K)), u.device, "r1")
    check(lib.lgr_r1_heads_colsum(_p(u), _p(dwpr), _p(ws), ws.numel(), B, K, _stream()), "lgr_r1_heads_colsum")
    return dwpr


# ------------------------------------------------------------------ relativistic pairing + R2 (objective.hip, r1.hip; include/littlegan_rel.h)
REL_SIDE_SELF, REL_SIDE_OTHER = 0, 1


def pair_heads_loss(p, z, z_ref, t_c, kind, side, w_pr, w_c, loss, dz, accumulate):
    """gan_heads_loss with the real / fake term taken on a pair of logits: t = z - z_ref (side 0, SELF: loss and gradient) or z_ref - z
    (side 1, OTHER: the gradient with respect to z alone, nothing added to the loss); z [n], z_ref [m] with n % m == 0, row i pairs with
    z_ref[i mod m]; kind 1 logistic, 2 hinge, 3 lsgan, each its role-0 function.  The attribute term (t_c, w_c) is bce_heads_loss's."""
    n, J = p.shape
    _chk(p, name="p")
    _chk(z, (n,), "z")
    _chk(z_ref, name="z_ref")
    _chk(dz, (n, J), "dz")
    _chk(loss, (1,), "loss")
    if t_c is not None:
        _chk(t_c, (n, J - 1), "t_c")
    check(_lib.load().lgrel_pair_heads_loss_fwd_bwd(_p(p), _p(z), _p(z_ref), _p(t_c), int(kind), int(side), float(w_pr), float(w_c),
                                                    _p(loss), _p(dz), n, int(z_ref.numel()), J - 1, int(accumulate), _stream()),
          "lgrel_pair_heads_loss_fwd_bwd")


def r12_seed(g, w_real, w_fake, loss=None, r1_loss=None, r2_loss=None):
    """r1_seed over g [2B, ...] with a weight per half: -> (u0 = (w_half / B) g, r2 [2B] = |g_b|^2); r1_loss = the real half's term,
    r2_loss = the fake half's, loss = (loss + r1 term) + r2 term.  The bits of two r1_seed calls on the halves."""
    _chk(g, name="g")
    if g.shape[0] % 2:
        raise ValueError(f"r12_seed: g must hold the two halves of a batch, got {g.shape[0]} rows")
    B = g.shape[0] // 2
    L = g.numel() // (2 * B)
    for t, nm in ((loss, "loss"), (r1_loss, "r1_loss"), (r2_loss, "r2_loss")):
        if t is not None:
            _chk(t, (1,), nm)
    u0 = torch.empty_like(g)
    r2 = torch.empty(2 * B, dtype=torch.float32, device=g.device)
    lib = _lib.load()
    ws = workspace(int(lib.lgrel_r12_workspace_bytes(B, L)), g.device, "r1")
    check(lib.lgrel_r12_seed(_p(g), _p(u0), _p(r2), _p(loss), _p(r1_loss), _p(r2_loss), float(w_real), float(w_fake), _p(ws), ws.numel(),
                             B, L, _stream()), "lgrel_r12_seed")
    return u0, r2


# ------------------------------------------------------------------ learning-rate schedule on the device (sched.hip, loss_optim.hip; include/littlegan_sched.h)
SCHED_CONSTANT, SCHED_LINEAR, SCHED_COSINE = 0, 1, 2


def _chk_sched(t, who):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (8,)):
        raise ValueError(f"{who}: the schedule's state is a contiguous fp32 [8] CUDA tensor, got {t.dtype} {t.device} {tuple(t.shape)}")
    return t


def sched_init(k0=0, device="cuda", out=None):
    """The schedule's state {k0, 0, 0, 0, 0, 0, 0, 0} (fp32 [8]: the int32 step counter, fp32 s, the rates of G, D, A, three reserved
    words), written by a one-block kernel from a launch scalar: no host-to-device copy."""
    if out is None:
        out = torch.empty(8, dtype=torch.float32, device=device)
    _chk_sched(out, "sched_init")
    check(_lib.load().lgsch_init(_p(out), int(k0), _stream()), "lgsch_init")
    return out


def sched_step(state, kind, warmup, decay_steps, final_ratio, lr_g, lr_d, lr_a):
    """One step of the schedule: state[1] = s(k), state[2:5] = the three base rates times s(k), then k += 1 (saturating).  kind 0
    constant, 1 linear, 2 cosine; decay_steps None under constant."""
    _chk_sched(state, "sched_step")
    check(_lib.load().lgsch_step(_p(state), int(kind), int(warmup), 0 if decay_steps is None else int(decay_steps), float(final_ratio),
                                 float(lr_g), float(lr_d), float(lr_a), _stream()), "lgsch_step")
    return state


def sched_read(state):
    """(k, s, lr_g, lr_d, lr_a) on the host.  Synchronises: for logs, checkpoints and tests, not for the step."""
    _chk_sched(state, "sched_read")
    host = state.detach().cpu()
    return (int(host.view(torch.int32)[0]),) + tuple(float(x) for x in host[1:5])


def _chk_rate(lr):
    if not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1):
        raise ValueError(f"lr: need a 1-element fp32 CUDA tensor, got {lr.dtype} {lr.device} numel={lr.numel()}")
    return lr


def sched_clip_adam_update(w, g, m, v, state, lr, b1, b2, eps, clip, gscale=1.0):
    """clip_adam_update with the rate read on the device: lr is a 1-element fp32 tensor (a view of the schedule's state)."""
    n = _chk_adam("sched_clip_adam_update", None, w, g, m, v)
    check(_lib.load().lgsch_clip_adam_update(_p(w), _p(g), _p(m), _p(v), n, _p(state), _p(_chk_rate(lr)), float(b1), float(b2),
                                             float(eps), float(clip), float(gscale), _stream()), "lgsch_clip_adam_update")


def sched_clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, ema_state, lr, b1, b2, eps, clip, gscale, decay):
    """clip_adam_ema_update with the rate read on the device: lr is a 1-element fp32 tensor (a view of the schedule's state)."""
    n = _chk_adam("sched_clip_adam_ema_update", state, w, g, m, v, ema, ema_state=ema_state)
    check(_lib.load().lgsch_clip_adam_ema_update(_p(w), _p(g), _p(m), _p(v), _p(ema), n, int(lo), int(hi), _p(state), _p(ema_state),
                                                 _p(_chk_rate(lr)), float(b1), float(b2), float(eps), float(clip), float(gscale),
                                                 float(decay), _stream()), "lgsch_clip_adam_ema_update")


# ------------------------------------------------------------------ global-norm gradient clipping and the non-finite step guard (gradguard.hip, loss_optim.hip; include/littlegan_guard.h)
GUARD_CHUNK, GUARD_MAX_PARTIALS = 16384, 1024      # GG_CHUNK, GG_MAX_PARTIALS


def _chk_guard(t, who):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (8,)):
        raise ValueError(f"{who}: the guard's record is a contiguous fp32 [8] CUDA tensor, got {t.dtype} {t.device} {tuple(t.shape)}")
    return t


def _chk_grad(g, who):
    if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.dim() == 1 and g.numel() >= 1):
        raise ValueError(f"{who}: need a contiguous 1-d fp32 CUDA tensor of at least one element, got {g.dtype} {g.device} {tuple(g.shape)}")
    return g


def _chk_partial(p, who):
    if not (p.is_cuda and p.dtype in (torch.uint8, torch.float64) and p.is_contiguous()):
        raise ValueError(f"{who}: the partials are a contiguous uint8 or fp64 CUDA tensor, got {p.dtype} {p.device}")
    return p


def guard_partials_count(n):
    """P(n) = min(1024, ceil(n / 16384)): the fp64 partials of a sum of squares over n elements (lgg_partials_count)."""
    return int(_lib.load().lgg_partials_count(int(n)))


def guard_workspace_bytes(n):
    """8 P(n): the bytes of those partials (lgg_workspace_bytes)."""
    return int(_lib.load().lgg_workspace_bytes(int(n)))


def guard_init(skipped=0, nonfinite=0, device="cuda", out=None):
    """The guard's record {N, eff, skip_now, skipped, nonfinite, c, 0, 0} (fp32 [8]; words 2..4 int32) with every word zero but the two
    counters, written by a one-block kernel from launch scalars: no host-to-device copy."""
    if out is None:
        out = torch.empty(8, dtype=torch.float32, device=device)
    _chk_guard(out, "guard_init")
    check(_lib.load().lgg_init(_p(out), int(skipped), int(nonfinite), _stream()), "lgg_init")
    return out


def guard_sumsq_partial(g, partial):
    """partial[:P(n)] (fp64) = the per-workgroup sums of squares of g, in the order include/littlegan_guard.h states; partial holds at least
    guard_workspace_bytes(n) bytes."""
    _chk_grad(g, "guard_sumsq_partial")
    _chk_partial(partial, "guard_sumsq_partial")
    check(_lib.load().lgg_sumsq_partial(_p(g), g.numel(), _p(partial), partial.numel() * partial.element_size(), _stream()),
          "lgg_sumsq_partial")
    return partial


def guard_finalise(partial, n, rec, gscale, clip_norm, skip):
    """The record of the n elements whose partials `partial` holds: S in index order, then N, c, eff, skip_now and the counters
    (lgg_finalise).  clip_norm 0 = no clipping."""
    _chk_partial(partial, "guard_finalise")
    _chk_guard(rec, "guard_finalise")
    if partial.numel() * partial.element_size() < guard_workspace_bytes(n):
        raise ValueError(f"guard_finalise: {partial.numel() * partial.element_size()} bytes of partials, n = {n} has {guard_workspace_bytes(n)}")
    check(_lib.load().lgg_finalise(_p(partial), int(n), _p(rec), float(gscale), float(clip_norm), int(bool(skip)), _stream()), "lgg_finalise")
    return rec


def guard_read(rec):
    """{N, eff, skip_now, skipped, nonfinite, c} of a record on the host.  Synchronises: for logs, checkpoints and tests, not for the step."""
    _chk_guard(rec, "guard_read")
    host = rec.detach().cpu()
    words = host.view(torch.int32)
    return dict(N=float(host[0]), eff=float(host[1]), skip_now=int(words[2]), skipped=int(words[3]), nonfinite=int(words[4]), c=float(host[5]))


def grad_sumsq(g):
    """S = the fp64 sum of the squares of g as the guard computes it: the device's partials, added in index order.  Synchronises."""
    _chk_grad(g, "grad_sumsq")
    ws = workspace(guard_workspace_bytes(g.numel()), g.device, "gradguard")
    guard_sumsq_partial(g, ws)
    s = 0.0
    for x in ws[:8 * guard_partials_count(g.numel())].view(torch.float64).cpu().tolist():
        s += x
    return s


def guard_clip_adam_update(w, g, m, v, state, lr, rec, b1, b2, eps, clip):
    """sched_clip_adam_update with the gradient scale (rec word 1) and the skip flag (rec word 2) read on the device."""
    n = _chk_adam("guard_clip_adam_update", state, w, g, m, v)
    check(_lib.load().lgg_clip_adam_update(_p(w), _p(g), _p(m), _p(v), n, _p(state), _p(_chk_rate(lr)), _p(_chk_guard(rec, "guard_clip_adam_update")),
                                          float(b1), float(b2), float(eps), float(clip), _stream()), "lgg_clip_adam_update")


def guard_clip_adam_ema_update(w, g, m, v, ema, lo, hi, state, ema_state, lr, rec, b1, b2, eps, clip, decay):
    """sched_clip_adam_ema_update with the gradient scale and the skip flag read on the device; a skipped step takes the average alone."""
    n = _chk_adam("guard_clip_adam_ema_update", state, w, g, m, v, ema, ema_state=ema_state)
    check(_lib.load().lgg_clip_adam_ema_update(_p(w), _p(g), _p(m), _p(v), _p(ema), n, int(lo), int(hi), _p(state), _p(ema_state),
                                              _p(_chk_rate(lr)), _p(_chk_guard(rec, "guard_clip_adam_ema_update")), float(b1), float(b2),
                                              float(eps), float(clip), float(decay), _stream()), "lgg_clip_adam_ema_update")


def guard_adam_advance(state, rec, b1, b2):
    """adam_advance unless the record says that this step is skipped."""
    _chk(state, (2,), "state")
    check(_lib.load().lgg_adam_advance(_p(state), _p(_chk_guard(rec, "guard_adam_advance")), float(b1), float(b2), _stream()), "lgg_adam_advance")


# ------------------------------------------------------------------ faded blur of D's inputs (dblur.hip; include/littlegan_blur.h)
def _chk_blur(t, who):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (4,)):
        raise ValueError(f"{who}: the blur's state is a contiguous fp32 [4] CUDA tensor {{k, sigma, 0, 0}} (blur_init)")
    return t


def blur_init(k0=0, device="cuda", out=None):
    """The blur's state {k0, 0, 0, 0} (fp32 [4]: the int32 step counter, fp32 sigma, two reserved words), written by a one-block kernel
    from a launch scalar: no host-to-device copy."""
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=device)
    _chk_blur(out, "blur_init")
    check(_lib.load().lgblur_init(_p(out), int(k0), _stream()), "lgblur_init")
    return out


def blur_step(state, sigma0, images_per_step, fade_images):
    """One step of the fade: state[1] = sigma(k) = sigma0 * max(1 - k * images_per_step / fade_images, 0) (fp64, one conversion), then
    k += 1 (saturating).  See include/littlegan_blur.h"""
    _chk_blur(state, "blur_step")
    check(_lib.load().lgblur_step(_p(state), float(sigma0), int(images_per_step), int(fade_images), _stream()), "lgblur_step")
    return state


def blur_read(state):
    """(k, sigma) on the host.  Synchronises: for logs, checkpoints and tests, not for the step."""
    _chk_blur(state, "blur_read")
    host = state.detach().cpu()
    return int(host.view(torch.int32)[0]), float(host[1])


def blur_apply(x, state, out=None):
    """Blur(x): x [rows, S, S, 3] fp32 filtered with the Gaussian of sigma = state[1] (read on the device; radius min(floor(3 sigma), 30),
    zero fill), R == 0 a copy.  The operator is its own adjoint: the same call on an image gradient is the backward pass."""
    _chk(x, name="image")
    rows, S, W, c = x.shape
    if W != S or c != 3:
        raise ValueError(f"lgblur_apply: square 3-channel NHWC images only, got {tuple(x.shape)}")
    _chk_blur(state, "blur_apply")
    if out is None:
        out = torch.empty_like(x)
    _chk(out, x.shape, "out")
    check(_lib.load().lgblur_apply(_p(x), _p(state), _p(out), rows, S, _stream()), "lgblur_apply")
    return out
