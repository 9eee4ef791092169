"""Host side of the engine above the C-ABI: plan cache + autograd Functions.

PyTorch is plumbing here (device memory, streams, autograd graph); every arithmetic step
of the hot path runs in libsc_engine.so (hand-written HIP, include/sc_engine.h).
"""
import atexit
import collections
import math
import threading

import torch

from . import _lib
from .modes import kept_block

SC_PLAN_COMPLEX = _lib.SC_PLAN_COMPLEX
SC_PLAN_IO_BF16 = _lib.SC_PLAN_IO_BF16
_PLAN_LOCK = threading.Lock()
_PLANS = collections.OrderedDict()     # least recently used first; the key starts with the device index
MAX_CACHED_PLANS = 512                 # PER DEVICE.  Variable-resolution / incremental-mode training creates a plan per
                                       # (grid, kept modes, frequency map); a plan is a few KB .. MB of device tables
_RETIRED = collections.deque()         # (event, handle) of evicted plans: freed on a later cache MISS once the event
                                       # has passed -- never inline on the hit path (sc_plan_destroy = hipFree = a
                                       # device-wide synchronisation)
_NO_BF16_IO = set()       # (device, spatial, kept, norm, flags) the engine has no bfloat16-I/O kernels for


def _require_gpu(t, what="input"):
    if not t.is_cuda:
        raise RuntimeError(
            f"neuraloperator_amd: {what} is on {t.device}; the SpectralConv engine runs on "
            "MI355X (ROCm) devices only and has no CPU path -- move the module and its inputs "
            "to a 'cuda' device.")


def _freeze(freq):
    if freq is None:
        return None
    return tuple(None if f is None else tuple(f) for f in freq)


def get_plan(device, spatial, kept, fft_norm="forward", flags=0, freq=None, real_col=0):
    """Cached ``sc_plan`` for (device, spatial sizes, kept modes, norm, frequency maps)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           tuple(int(s) for s in spatial), tuple(int(k) for k in kept), fft_norm, flags,
           _freeze(freq), int(real_col))
    with _PLAN_LOCK:
        plan = _PLANS.get(key)
        if plan is None:
            lib = _lib.get_lib()
            with torch.cuda.device(key[0]):
                plan = lib.plan_create(key[1], key[2], fft_norm=fft_norm, flags=flags, freq=freq,
                                       real_col=real_col)
            _PLANS[key] = plan
            _evict_and_reap(key[0])
        else:
            _PLANS.move_to_end(key)
    return plan


def _evict_and_reap(dev_index):
    """Called under _PLAN_LOCK on a cache miss (plan creation has just allocated and copied, i.e. already paid a
    synchronising call).  Plans of `dev_index` beyond the per-device cap are RETIRED behind an event recorded on the
    current stream; retired plans whose event has completed are released (their handle frees the device tables once
    no autograd context references it any more)."""
    mine = [k for k in _PLANS if k[0] == dev_index]
    for k in mine[:max(len(mine) - MAX_CACHED_PLANS, 0)]:          # least recently used first
        ev = None
        if torch.cuda.is_available():
            with torch.cuda.device(dev_index):
                ev = torch.cuda.Event()
                ev.record()
        _RETIRED.append((ev, _PLANS.pop(k)))
    for _ in range(len(_RETIRED)):
        ev, handle = _RETIRED.popleft()
        if ev is None or ev.query():
            del handle
        else:
            _RETIRED.append((ev, handle))


def get_plan_bf16_io(device, spatial, kept, fft_norm, flags):
    """Plan whose real tensors are bfloat16 in memory (SC_PLAN_IO_BF16), or None where the engine only has
    float32 I/O for the shape (everything off the fused 2-D kernels): the caller then converts."""
    key = (device.index, tuple(int(s) for s in spatial), tuple(int(k) for k in kept), fft_norm, flags)
    if key in _NO_BF16_IO:
        return None
    try:
        return get_plan(device, spatial, kept, fft_norm, flags | SC_PLAN_IO_BF16)
    except _lib.EngineError as e:
        if "SC_PLAN_IO_BF16 is implemented" not in str(e):
            raise                       # out of memory, HIP errors, ...: not a property of the shape
        _NO_BF16_IO.add(key)
        return None


@atexit.register
def _destroy_plans():
    # device memory is reclaimed with the process: the handles are dropped without calling into the library
    # (_lib marks the shutdown first: atexit handlers run in reverse order of registration, _lib is imported earlier)
    _lib._SHUTDOWN = True
    _PLANS.clear()
    _RETIRED.clear()


def _stream():
    # the raw handle of torch's current stream: torch.cuda.current_stream().cuda_stream builds a Stream object per call
    # (~12 us of host time, four to a dozen calls per layer step)
    try:
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
    except AttributeError:                                      # a torch build without the private accessor
        return torch.cuda.current_stream().cuda_stream


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


class SpectralConvDenseFn(torch.autograd.Function):
    """y = irfftn(pad(einsum('bi..,io..->bo..', trunc(rfftn(x)), W))) + bias, one C-ABI call
    each way (sc_layer_forward / sc_layer_backward).

    Replaces /root/reference/neuralop/layers/spectral_convolution.py:443-568 and the
    autograd graph PyTorch derives from it."""

    @staticmethod
    def forward(ctx, x, weight, bias, n_modes_attr, max_n_modes_attr, fft_norm, flags):
        _require_gpu(x)
        _require_gpu(weight, "weight")
        lib = _lib.get_lib()
        x = x.contiguous()
        w = weight.detach()
        if w.dtype != torch.complex64:
            w = w.to(torch.complex64)
        w = w.contiguous()
        b, cin = x.shape[:2]
        cout = w.shape[1]
        if w.shape[0] != cin:
            raise ValueError(f"input has {cin} channels, weight expects {w.shape[0]}")
        spatial = list(x.shape[2:])
        kept, w_start = kept_block(spatial, n_modes_attr, max_n_modes_attr)
        # bfloat16 activations: the fused kernels read / write them as they are (fp32 arithmetic, y and
        # gx rounded once on the store); other shapes and dtypes are converted to float32 here
        plan = get_plan_bf16_io(x.device, spatial, kept, fft_norm, flags) if x.dtype == torch.bfloat16 else None
        io_dtype = torch.bfloat16 if plan is not None else torch.float32
        if plan is None:
            x = x.float()
            plan = get_plan(x.device, spatial, kept, fft_norm, flags)
        L = lib.layer_desc(b, cin, cout, list(w.shape[2:]), w_start)
        with torch.cuda.device(x.device):
            ws = _ws(lib.layer_workspace_bytes(plan, L), x.device)
            y = torch.empty((b, cout, *spatial), dtype=io_dtype, device=x.device)
            xhat = torch.empty((b, cin, *kept, 2), dtype=torch.float32, device=x.device)
            bias_flat = None
            if bias is not None:
                bias_flat = bias.detach().reshape(-1).float().contiguous()
            lib.layer_forward(plan, L, x.data_ptr(), torch.view_as_real(w).data_ptr(),
                              0 if bias_flat is None else bias_flat.data_ptr(),
                              y.data_ptr(), xhat.data_ptr(), ws.data_ptr(), _stream())
        ctx.save_for_backward(xhat, w)
        ctx.plan, ctx.L = plan, L
        ctx.io_dtype = io_dtype
        ctx.x_shape = tuple(x.shape)
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        ctx.w_shape = tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.get_lib()
        xhat, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        gy = gy.contiguous()
        if gy.dtype != ctx.io_dtype:
            gy = gy.to(ctx.io_dtype)
        dev = gy.device
        with torch.cuda.device(dev):
            ws = _ws(lib.layer_workspace_bytes(ctx.plan, ctx.L), dev)
            gx = torch.empty(ctx.x_shape, dtype=ctx.io_dtype, device=dev) if need_x else None
            gw = None
            if need_w:
                full = all(ctx.L.w_start[d] == 0 for d in range(len(ctx.w_shape) - 2)) and \
                    tuple(xhat.shape[2:-1]) == tuple(ctx.w_shape[2:])
                alloc = torch.empty if full else torch.zeros
                gw = alloc((*ctx.w_shape, 2), dtype=torch.float32, device=dev)
            gb = None
            if need_b and ctx.bias_shape is not None:
                gb = torch.empty(ctx.L.cout, dtype=torch.float32, device=dev)
            lib.layer_backward(ctx.plan, ctx.L, gy.data_ptr(), xhat.data_ptr(),
                               torch.view_as_real(w).data_ptr(),
                               0 if gx is None else gx.data_ptr(),
                               0 if gw is None else gw.data_ptr(),
                               0 if gb is None else gb.data_ptr(), ws.data_ptr(), _stream())
        gw_c = torch.view_as_complex(gw) if gw is not None else None
        gb_r = gb.reshape(ctx.bias_shape) if gb is not None else None
        return gx, gw_c, gb_r, None, None, None, None


class FourierLayerFn(torch.autograd.Function):
    """out = act(spectral_conv(x) + skip): the Fourier layer of an FNO block (neuralop/layers/fno_block.py:392-414:
    ``x_fno + x_skip_fno`` followed by the non-linearity) with the addition and the activation done in the store
    path of the inverse transform -- ``sc_layer_forward_ex``.  ``act``: "gelu" (exact, torch's
    default) or None.  Backward: the activation's derivative is one elementwise pass over the saved pre-activation
    (ATen's gelu_backward), its result is both the skip branch's gradient and the input of ``sc_layer_backward``."""

    @staticmethod
    def forward(ctx, x, weight, bias, skip, act, n_modes_attr, max_n_modes_attr, fft_norm, flags):
        _require_gpu(x)
        _require_gpu(weight, "weight")
        lib = _lib.get_lib()
        if act not in (None, "gelu"):
            raise ValueError(f"activation {act!r}: the fused epilogue knows 'gelu' and None")
        x = x.contiguous().float()
        skip = skip.contiguous().float()
        w = weight.detach().to(torch.complex64).contiguous()
        b, cin = x.shape[:2]
        cout = w.shape[1]
        spatial = list(x.shape[2:])
        if tuple(skip.shape) != (b, cout, *spatial):
            raise ValueError(f"skip has shape {tuple(skip.shape)}, the layer's output is {(b, cout, *spatial)}")
        kept, w_start = kept_block(spatial, n_modes_attr, max_n_modes_attr)
        plan = get_plan(x.device, spatial, kept, fft_norm, flags)
        L = lib.layer_desc(b, cin, cout, list(w.shape[2:]), w_start)
        need_pre = act == "gelu" and any(ctx.needs_input_grad[:4])
        with torch.cuda.device(x.device):
            ws = _ws(lib.layer_workspace_bytes(plan, L), x.device)
            y = torch.empty((b, cout, *spatial), dtype=torch.float32, device=x.device)
            pre = torch.empty_like(y) if need_pre else None
            xhat = torch.empty((b, cin, *kept, 2), dtype=torch.float32, device=x.device)
            bias_flat = None if bias is None else bias.detach().reshape(-1).float().contiguous()
            lib.layer_forward_ex(plan, L, x.data_ptr(), torch.view_as_real(w).data_ptr(),
                                 0 if bias_flat is None else bias_flat.data_ptr(), skip.data_ptr(),
                                 0 if pre is None else pre.data_ptr(),
                                 _lib.SC_ACT_GELU if act == "gelu" else _lib.SC_ACT_NONE,
                                 y.data_ptr(), xhat.data_ptr(), ws.data_ptr(), _stream())
        ctx.save_for_backward(xhat, w, pre)
        ctx.plan, ctx.L, ctx.act = plan, L, act
        ctx.x_shape, ctx.w_shape = tuple(x.shape), tuple(weight.shape)
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        return y

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.get_lib()
        xhat, w, pre = ctx.saved_tensors
        need_x, need_w, need_b, need_s = ctx.needs_input_grad[:4]
        gz = gout.contiguous().float()
        if ctx.act == "gelu":
            gz = torch.ops.aten.gelu_backward(gz, pre)              # host glue: one elementwise pass
        dev = gz.device
        gx = gw = gb = None
        if need_x or need_w or (need_b and ctx.bias_shape is not None):
            with torch.cuda.device(dev):
                ws = _ws(lib.layer_workspace_bytes(ctx.plan, ctx.L), dev)
                gx = torch.empty(ctx.x_shape, dtype=torch.float32, device=dev) if need_x else None
                if need_w:
                    full = all(ctx.L.w_start[d] == 0 for d in range(len(ctx.w_shape) - 2)) and \
                        tuple(xhat.shape[2:-1]) == tuple(ctx.w_shape[2:])
                    gw = (torch.empty if full else torch.zeros)((*ctx.w_shape, 2), dtype=torch.float32, device=dev)
                if need_b and ctx.bias_shape is not None:
                    gb = torch.empty(ctx.L.cout, dtype=torch.float32, device=dev)
                lib.layer_backward(ctx.plan, ctx.L, gz.data_ptr(), xhat.data_ptr(), torch.view_as_real(w).data_ptr(),
                                   0 if gx is None else gx.data_ptr(), 0 if gw is None else gw.data_ptr(),
                                   0 if gb is None else gb.data_ptr(), ws.data_ptr(), _stream())
        return (gx, None if gw is None else torch.view_as_complex(gw),
                None if gb is None else gb.reshape(ctx.bias_shape), gz if need_s else None,
                None, None, None, None, None)


class TransformForwardFn(torch.autograd.Function):
    """x (B, C, d1..dN) real -> truncated spectrum (B, C, k1..kN) complex (weight order).
    forward = SC_FWD_SCALED, backward = its adjoint SC_INV_ADJ_R2C."""

    @staticmethod
    def forward(ctx, x, kept, fft_norm, flags, freq=None):
        _require_gpu(x)
        lib = _lib.get_lib()
        cplx = bool(flags & _lib.SC_PLAN_COMPLEX)
        if cplx:
            x = torch.view_as_real(x.contiguous().to(torch.complex64)).contiguous()
            spatial = list(x.shape[2:-1])
        else:
            x = x.contiguous().float()
            spatial = list(x.shape[2:])
        b, c = x.shape[:2]
        plan = get_plan(x.device, spatial, kept, fft_norm, flags, freq)
        with torch.cuda.device(x.device):
            ws = _ws(lib.plan_workspace_bytes(plan, b * c), x.device)
            xhat = torch.empty((b, c, *kept, 2), dtype=torch.float32, device=x.device)
            lib.transform_forward(plan, _lib.SC_FWD_SCALED, x.data_ptr(), xhat.data_ptr(), b * c,
                                  ws.data_ptr(), _stream())
        ctx.plan = plan
        ctx.x_shape = tuple(x.shape)
        ctx.cplx = cplx
        return torch.view_as_complex(xhat)

    @staticmethod
    def backward(ctx, gxhat):
        lib = _lib.get_lib()
        g = torch.view_as_real(gxhat.contiguous().to(torch.complex64)).contiguous()
        b, c = ctx.x_shape[:2]
        with torch.cuda.device(g.device):
            ws = _ws(lib.plan_workspace_bytes(ctx.plan, b * c), g.device)
            gx = torch.empty(ctx.x_shape, dtype=torch.float32, device=g.device)
            lib.transform_inverse(ctx.plan, _lib.SC_INV_ADJ_R2C, g.data_ptr(), 0, c, gx.data_ptr(),
                                  b * c, ws.data_ptr(), _stream())
        if ctx.cplx:
            gx = torch.view_as_complex(gx)
        return gx, None, None, None, None


class TransformInverseFn(torch.autograd.Function):
    """truncated spectrum (B, C, k..) complex -> y (B, C, d..) real (+ bias).
    forward = SC_INV_PADDED, backward = its adjoint SC_FWD_ADJ_C2R (bias grad from DC)."""

    @staticmethod
    def forward(ctx, yhat, bias, spatial, fft_norm, flags, freq=None, real_col=0):
        _require_gpu(yhat)
        lib = _lib.get_lib()
        cplx = bool(flags & _lib.SC_PLAN_COMPLEX)
        if cplx and bias is not None:
            raise ValueError("complex-data inverse transform takes no bias (add it afterwards)")
        yh = torch.view_as_real(yhat.contiguous().to(torch.complex64)).contiguous()
        b, c = yh.shape[:2]
        kept = list(yh.shape[2:-1])
        plan = get_plan(yh.device, spatial, kept, fft_norm, flags, freq, real_col)
        with torch.cuda.device(yh.device):
            ws = _ws(lib.plan_workspace_bytes(plan, b * c), yh.device)
            y = torch.empty((b, c, *spatial) + ((2,) if cplx else ()), dtype=torch.float32, device=yh.device)
            bias_flat = None if bias is None else bias.detach().reshape(-1).float().contiguous()
            lib.transform_inverse(plan, _lib.SC_INV_PADDED, yh.data_ptr(),
                                  0 if bias_flat is None else bias_flat.data_ptr(), c,
                                  y.data_ptr(), b * c, ws.data_ptr(), _stream())
        ctx.plan = plan
        ctx.kept = kept
        ctx.cplx = cplx
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        return torch.view_as_complex(y) if cplx else y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.get_lib()
        if ctx.cplx:
            gy = torch.view_as_real(gy.contiguous().to(torch.complex64)).contiguous()
        else:
            gy = gy.contiguous().float()
        b, c = gy.shape[:2]
        with torch.cuda.device(gy.device):
            ws = _ws(lib.plan_workspace_bytes(ctx.plan, b * c), gy.device)
            ghat = torch.empty((b, c, *ctx.kept, 2), dtype=torch.float32, device=gy.device)
            lib.transform_forward(ctx.plan, _lib.SC_FWD_ADJ_C2R, gy.data_ptr(), ghat.data_ptr(),
                                  b * c, ws.data_ptr(), _stream())
            gb = None
            if ctx.bias_shape is not None and ctx.needs_input_grad[1]:
                gb = torch.empty(c, dtype=torch.float32, device=gy.device)
                lib.bias_grad(ctx.plan, ghat.data_ptr(), b, c, gb.data_ptr(), _stream())
                gb = gb.reshape(ctx.bias_shape)
        return torch.view_as_complex(ghat), gb, None, None, None, None, None


def _cview(t):
    """complex64 contiguous tensor -> float32 view pointer holder."""
    t = t.to(torch.complex64) if t.dtype != torch.complex64 else t
    return torch.view_as_real(t.contiguous())


def modegemm(a, b, *, P, Q, R, n_modes, a_strides, b_strides, out, c_strides, conj_a=False,
             conj_b=False, b_idx=None, c_idx=None, accumulate=False):
    """Raw mode-batched complex GEMM (sc_modegemm).  ``a``, ``b``, ``out`` are complex64 CUDA
    tensors; strides are (sp, sr, sm) / (sr, sq, sm) / (sp, sq, sm) in complex elements."""
    lib = _lib.get_lib()
    av, bv, cv = torch.view_as_real(a), torch.view_as_real(b), torch.view_as_real(out)
    with torch.cuda.device(out.device):
        lib.modegemm(av.data_ptr(), bv.data_ptr(), cv.data_ptr(), _stream(),
                     P=P, Q=Q, R=R, n_modes=n_modes,
                     a_sp=a_strides[0], a_sr=a_strides[1], a_sm=a_strides[2],
                     b_sr=b_strides[0], b_sq=b_strides[1], b_sm=b_strides[2],
                     c_sp=c_strides[0], c_sq=c_strides[1], c_sm=c_strides[2],
                     conj_a=int(conj_a), conj_b=int(conj_b), accumulate=int(accumulate),
                     b_idx=0 if b_idx is None else b_idx.data_ptr(),
                     c_idx=0 if c_idx is None else c_idx.data_ptr())
    return out


def dense_contract_backward(xhat, w, g, need_x=True, need_w=True):
    """The two autograd einsums of 'bixy,ioxy->boxy' (spectral_convolution.py:21-46):
    gxhat[b,i,m] = sum_o g[b,o,m] conj(w[i,o,m]),  gw[i,o,m] = sum_b conj(xhat[b,i,m]) g[b,o,m]
    on contiguous (b, c, modes...) complex64 blocks.  When both are wanted they go down as ONE call
    (sc_modegemm_pair: one launch of k_modegemm_dma_bwd when the pair qualifies, else two launches)."""
    b, ci = xhat.shape[:2]
    co = w.shape[1]
    mk = xhat[0, 0].numel()
    gx = gw = None
    if need_x and need_w and b and ci and co and mk:
        kw_w = dict(P=ci, Q=co, R=b, n_modes=mk, a_sp=mk, a_sr=ci * mk, a_sm=1, conj_a=1,
                    b_sr=co * mk, b_sq=mk, b_sm=1, c_sp=co * mk, c_sq=mk, c_sm=1)
        kw_x = dict(P=b, Q=ci, R=co, n_modes=mk, a_sp=co * mk, a_sr=mk, a_sm=1,
                    b_sr=mk, b_sq=co * mk, b_sm=1, conj_b=1, c_sp=ci * mk, c_sq=mk, c_sm=1)
        gx, gw = torch.empty_like(xhat), torch.empty_like(w)
        ptr = lambda t: torch.view_as_real(t).data_ptr()
        with torch.cuda.device(g.device):
            _lib.get_lib().modegemm_pair(kw_w, ptr(xhat), ptr(g), ptr(gw), kw_x, ptr(g), ptr(w), ptr(gx), _stream())
        return gx, gw
    if need_x:
        gx = torch.empty_like(xhat)
        modegemm(g, w, P=b, Q=ci, R=co, n_modes=mk, a_strides=(co * mk, mk, 1), b_strides=(mk, co * mk, 1),
                 conj_b=True, out=gx, c_strides=(ci * mk, mk, 1))
    if need_w:
        gw = torch.empty_like(w)
        modegemm(xhat, g, P=ci, Q=co, R=b, n_modes=mk, a_strides=(mk, ci * mk, 1), conj_a=True,
                 b_strides=(co * mk, mk, 1), out=gw, c_strides=(co * mk, mk, 1))
    return gx, gw


class ModeContractDenseFn(torch.autograd.Function):
    """yhat[b,o,m] = sum_i xhat[b,i,m] * w[i,o,m] on an arbitrary (e.g. mode-sharded) block of
    modes; w has exactly the mode extents of xhat.  Three sc_modegemm launches in total
    (forward, gX, gW) -- the einsum 'bixy,ioxy->boxy' of spectral_convolution.py:21-46 and its
    two autograd einsums."""

    @staticmethod
    def forward(ctx, xhat, w):
        _require_gpu(xhat, "xhat")
        xhat = xhat.contiguous().to(torch.complex64)
        w = w.contiguous().to(torch.complex64)
        b, ci = xhat.shape[:2]
        co = w.shape[1]
        if tuple(w.shape[2:]) != tuple(xhat.shape[2:]) or w.shape[0] != ci:
            raise ValueError(f"weight block {tuple(w.shape)} does not match spectrum {tuple(xhat.shape)}")
        mk = 1
        for k in xhat.shape[2:]:
            mk *= int(k)
        yhat = torch.empty((b, co, *xhat.shape[2:]), dtype=torch.complex64, device=xhat.device)
        modegemm(xhat, w, P=b, Q=co, R=ci, n_modes=mk, a_strides=(ci * mk, mk, 1),
                 b_strides=(co * mk, mk, 1), out=yhat, c_strides=(co * mk, mk, 1))
        ctx.save_for_backward(xhat, w)
        ctx.dims = (b, ci, co, mk)
        return yhat

    @staticmethod
    def backward(ctx, g):
        xhat, w = ctx.saved_tensors
        b, ci, co, mk = ctx.dims
        g = g.contiguous().to(torch.complex64)
        gx, gw = dense_contract_backward(xhat, w, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw


# ------------------------------------------------------------------------------------------
# generic mode GEMM with autograd: the pairwise steps of the factorized contractions
# ------------------------------------------------------------------------------------------
# row count from which the gradient steps of ModeGemmFn re-label a long reduction onto the lanes
# (tests set it to 1 to force those paths at fixture sizes)
RELABEL_MIN_ROWS = 4096


def _strides3(t, lead):
    """(s0, s1, sm) in complex elements of a [lead0, lead1, M] or [lead0, lead1] (mode-independent) view."""
    if t.dim() == 3:
        return int(t.stride(0)), int(t.stride(1)), int(t.stride(2))
    return int(t.stride(0)), int(t.stride(1)), 0


def _raw_mode_gemm(a, b, n_modes, conj_a, conj_b, reduce_modes=False, flags=0):
    """a: [P, R, M] or [P, R]; b: [R, Q, M] or [R, Q]; complex64 CUDA tensors/views (any strides).
    Returns C[P, Q, M] (or C[P, Q] = sum over modes when reduce_modes)."""
    lib = _lib.get_lib()
    # the lanes run over the modes: an operand whose mode stride is not 1 would be gathered
    if a.dim() == 3 and a.stride(2) != 1 and a.shape[2] > 1:
        a = a.contiguous()
    if b.dim() == 3 and b.stride(2) != 1 and b.shape[2] > 1:
        b = b.contiguous()
    P, R = int(a.shape[0]), int(a.shape[1])
    Q = int(b.shape[1])
    a_sp, a_sr, a_sm = _strides3(a, 2)
    b_sr, b_sq, b_sm = _strides3(b, 2)
    dev = a.device
    with torch.cuda.device(dev):
        if reduce_modes:
            kw = dict(P=P, Q=Q, R=R, n_modes=n_modes, a_sp=a_sp, a_sr=a_sr, a_sm=a_sm, b_sr=b_sr, b_sq=b_sq, b_sm=b_sm,
                      conj_a=int(conj_a), conj_b=int(conj_b), flags=int(flags), c_sp=Q, c_sq=1, c_sm=0)
            ws_bytes = lib.modegemm_msum_workspace_bytes(**kw) if P and Q and n_modes and R else 0
            if ws_bytes:
                # matrix-core kernel + fixed-order reduction (sc_kernels_fmx.h): C is overwritten, no zero fill
                out = torch.empty((P, Q), dtype=torch.complex64, device=dev)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                lib.modegemm_msum_ws(a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes, _stream(), **kw)
                return out
            out = torch.zeros((P, Q), dtype=torch.complex64, device=dev)
            fn, c = lib.modegemm_msum, dict(c_sp=Q, c_sq=1, c_sm=0)
        else:
            out = torch.empty((P, Q, n_modes), dtype=torch.complex64, device=dev)
            fn, c = lib.modegemm, dict(c_sp=Q * n_modes, c_sq=n_modes, c_sm=1)
        if P and Q and n_modes:
            fn(a.data_ptr(), b.data_ptr(), out.data_ptr(), _stream(), P=P, Q=Q, R=R, n_modes=n_modes,
               a_sp=a_sp, a_sr=a_sr, a_sm=a_sm, b_sr=b_sr, b_sq=b_sq, b_sm=b_sm,
               conj_a=int(conj_a), conj_b=int(conj_b), flags=int(flags), **c)
    return out


class ModeGemmFn(torch.autograd.Function):
    """C[p,q,m] = sum_r opA(A)[p,r,m] * opB(B)[r,q,m] with either operand possibly mode-independent
    (a 2-D tensor: Tucker / CP factor matrices).  Forward and both gradients run on sc_modegemm /
    sc_modegemm_msum (gradient of a mode-independent operand = sum over the modes: wave reduction).
    One pairwise step of the reference's _contract_tucker / _contract_cp einsums
    (spectral_convolution.py:55-103) and of their autograd."""

    @staticmethod
    def forward(ctx, a, b, n_modes, conj_a, conj_b, flags=0):
        _require_gpu(a, "A")
        _require_gpu(b, "B")
        a = a if a.dtype == torch.complex64 else a.to(torch.complex64)
        b = b if b.dtype == torch.complex64 else b.to(torch.complex64)
        if a.shape[1] != b.shape[0]:
            raise ValueError(f"inner extents differ: A {tuple(a.shape)} B {tuple(b.shape)}")
        ctx.save_for_backward(a, b)
        ctx.cfg = (int(n_modes), bool(conj_a), bool(conj_b))
        ctx.flags = int(flags)                # SC_GEMM_F16: the complex-half contraction, forward AND gradients
        if ctx.flags & _lib.SC_GEMM_F16 and (a.dim() != 3 or b.dim() != 3):
            raise ValueError("SC_GEMM_F16 contracts two per-mode operands (the dense equation)")
        return _raw_mode_gemm(a, b, int(n_modes), conj_a, conj_b, flags=ctx.flags)

    @staticmethod
    def backward(ctx, gc):
        a, b = ctx.saved_tensors
        M, ca, cb = ctx.cfg
        gc = gc.contiguous()
        P, R, Q = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
        ga = gb = None
        if ctx.needs_input_grad[0]:
            # grad_a = sum_q gC * conj(opB(B)); conj_a: grad_A = conj(grad_a) = sum_q conj(gC) * opB(B)
            cbx = cb if ca else not cb
            if a.dim() == 2 and b.dim() == 3 and P >= RELABEL_MIN_ROWS and M < 64:
                # A is mode independent and tall, the modes are few (core x last-mode-factor step of a Tucker
                # weight: 46656 x 19 against 33 modes): a plain (P x QM)(QM x R) product with the ROWS on the
                # lanes instead of a 33-lane wave reduction per row -- 128 -> ~25 us
                gt = gc.reshape(P, Q * M).t().contiguous().unsqueeze(0)                # [1, QM, P]
                bm = b.permute(1, 2, 0).reshape(Q * M, R)                              # [QM, R], mode independent
                ga = _raw_mode_gemm(gt, bm, P, ca, cbx).reshape(R, P).t()
            else:
                ga = _raw_mode_gemm(gc, b.transpose(0, 1), M, ca, cbx, reduce_modes=(a.dim() == 2), flags=ctx.flags)
        if ctx.needs_input_grad[1]:
            # grad_b = sum_p conj(opA(A)) * gC; conj_b: grad_B = conj(grad_b) = sum_p opA(A) * conj(gC)
            cax = ca if cb else not ca
            if a.dim() == 2 and b.dim() == 3 and P >= 8 * Q * M:
                # long reduction over p, few outputs (core x last-mode-factor step of a Tucker weight):
                # put p on the lanes -- sc_modegemm_msum with modes := p, columns := (q, m) -- instead
                # of a handful of workgroups walking all of p serially (21.7 ms -> ~0.1 ms at rank 0.1);
                # both operands are laid out with p contiguous first (a strided view gathers: 296 -> ~30 us)
                a2 = a.t().contiguous().unsqueeze(1)                                    # [R, 1, P]
                g2 = gc.reshape(P, Q * M).t().contiguous().unsqueeze(0)                 # [1, Q M, P]
                gb = _raw_mode_gemm(a2, g2, P, cax, cb, reduce_modes=True).reshape(R, Q, M)
            elif b.dim() == 2 and a.dim() == 3 and P * M >= RELABEL_MIN_ROWS and P >= 8 * R:
                # B is mode independent and the sum runs over many rows p AND the modes (mode-factor step:
                # 1296 rows x 33 modes -> a 36 x 64 gradient): (p, m) jointly on the lanes, 430 -> ~40 us
                a2 = a.permute(1, 0, 2).reshape(R, 1, P * M)                            # [R, 1, (p m)] (copy)
                g2 = gc.permute(1, 0, 2).reshape(1, Q, P * M)                           # [1, Q, (p m)] (copy)
                gb = _raw_mode_gemm(a2, g2, P * M, cax, cb, reduce_modes=True)
            else:
                gb = _raw_mode_gemm(a.transpose(0, 1), gc, M, cax, cb, reduce_modes=(b.dim() == 2), flags=ctx.flags)
        return ga, gb, None, None, None, None


class TuckerModes2dFn(torch.autograd.Function):
    """T[f, g, x, y] = sum_{c, d} core[f, g, c, d] U_x[x, c] U_y[y, d] and its three gradients, one launch each way
    (sc_tucker_modes_forward / _backward): the batch-independent part of the 2-D Tucker contraction
    (spectral_convolution.py:76-103)."""

    @staticmethod
    def forward(ctx, core, ux, uy):
        _require_gpu(core, "core")
        lib = _lib.get_lib()
        f, g, rx, ry = (int(v) for v in core.shape)
        mx, my = int(ux.shape[0]), int(uy.shape[0])
        c, a, b = (t.detach().to(torch.complex64).contiguous() for t in (core, ux, uy))
        out = torch.empty((f, g, mx * my), dtype=torch.complex64, device=core.device)
        with torch.cuda.device(core.device):
            lib.tucker_modes_forward(f * g, rx, ry, mx, my, torch.view_as_real(c).data_ptr(), torch.view_as_real(a).data_ptr(),
                                     torch.view_as_real(b).data_ptr(), torch.view_as_real(out).data_ptr(), _stream())
        ctx.save_for_backward(c, a, b)
        return out

    @staticmethod
    def backward(ctx, gt):
        c, a, b = ctx.saved_tensors
        lib = _lib.get_lib()
        f, g, rx, ry = (int(v) for v in c.shape)
        mx, my = int(a.shape[0]), int(b.shape[0])
        gt = gt.to(torch.complex64).contiguous()
        gc, ga, gb = torch.empty_like(c), torch.empty_like(a), torch.empty_like(b)
        ws = torch.empty(lib.tucker_modes_workspace_bytes(f * g, rx, ry, mx, my), dtype=torch.uint8, device=c.device)
        p = lambda t: torch.view_as_real(t).data_ptr()
        with torch.cuda.device(c.device):
            lib.tucker_modes_backward(f * g, rx, ry, mx, my, p(c), p(a), p(b), p(gt), p(gc), p(ga), p(gb), ws.data_ptr(),
                                      _stream())
        return gc, ga, gb


def tucker_modes_2d(core, ux, uy):
    """None when the sizes are outside the kernel's limits (the caller then takes the chain of mode GEMMs)."""
    f, g, rx, ry = (int(v) for v in core.shape)
    if not _lib.get_lib().tucker_modes_supported(f * g, rx, ry, int(ux.shape[0]), int(uy.shape[0])):
        return None
    return TuckerModes2dFn.apply(core, ux, uy)


class TuckerChainFn(torch.autograd.Function):
    """The activation side of the factorized Tucker contraction as ONE autograd node (round 3):
        z[b,f,m] = sum_i xhat[b,i,m] U_in[i,f];  t[b,g,m] = sum_f z[b,f,m] T[f,g,m];  yhat[b,o,m] = sum_g t[b,g,m] U_out[o,g]
    (the pairwise order of _forward_tucker, spectral_convolution.py:76-103) -- the same launches as three ModeGemmFn
    nodes, but a step of this layer is ~30 launches of 20-100 us each and the host needs about as long to walk four
    autograd nodes and their views as the device needs to run them (scripts/tfno_cpu_bound.py: 0.62 ms to issue a
    0.77 ms step).  Session 2: ONE C-ABI call per direction (sc_tucker_chain_forward / _backward) issues the three /
    six products from C++.  Backward: the six products of the three nodes, in the order their gradients are needed."""

    @staticmethod
    def forward(ctx, xhat, u_in, t3, u_out):
        _require_gpu(xhat, "xhat")
        c64 = lambda v: (v if v.dtype == torch.complex64 else v.to(torch.complex64)).contiguous()
        xhat, u_in, t3, u_out = c64(xhat), c64(u_in), c64(t3), c64(u_out)
        b, ci, m = (int(v) for v in xhat.shape)
        r1, r2, co = int(u_in.shape[1]), int(u_out.shape[1]), int(u_out.shape[0])
        if tuple(t3.shape) != (r1, r2, m) or int(u_in.shape[0]) != ci:
            raise ValueError(f"tucker_chain: xhat {tuple(xhat.shape)} u_in {tuple(u_in.shape)} t3 {tuple(t3.shape)} "
                             f"u_out {tuple(u_out.shape)} do not chain")
        dev = xhat.device
        z = torch.empty((b, r1, m), dtype=torch.complex64, device=dev)
        t = torch.empty((b, r2, m), dtype=torch.complex64, device=dev)
        yhat = torch.empty((b, co, m), dtype=torch.complex64, device=dev)
        ctx.dims = (b, ci, co, r1, r2, m)
        ctx.fused = False
        t3m = None
        if b and m:
            lib = _lib.get_lib()
            with torch.cuda.device(dev):
                # round 5: ONE launch for the three products where the shape fits (batch <= 32, <= 64 channels, ranks <= 48,
                # extents multiples of 4 -- BASELINE configs[2]): a workgroup walks xhat -> z -> t -> yhat for four modes out of
                # LDS (csrc/sc_kernels_tkchain.h); t3m = the mode-major copy of t3 that call writes and the backward call reads
                ctx.fused = lib.tucker_chain_fused_supported(ctx.dims) and all(
                    v.data_ptr() % 16 == 0 for v in (xhat, z, t, yhat))
                if ctx.fused:
                    t3m = torch.empty((m, r1, r2), dtype=torch.complex64, device=dev)
                    lib.tucker_chain_forward_fused(ctx.dims, xhat.data_ptr(), u_in.data_ptr(), t3.data_ptr(), u_out.data_ptr(),
                                                   t3m.data_ptr(), z.data_ptr(), t.data_ptr(), yhat.data_ptr(), _stream())
                else:
                    # ONE host call for the three products (round 3, session 2: sc_tucker_chain_forward issues the same three
                    # sc_modegemm launches from C++; a factorized step was ~0.6-0.76 ms of interpreter time per 0.76 ms of
                    # device time)
                    lib.tucker_chain_forward(ctx.dims, xhat.data_ptr(), u_in.data_ptr(), t3.data_ptr(), u_out.data_ptr(),
                                             z.data_ptr(), t.data_ptr(), yhat.data_ptr(), _stream())
        if t3m is not None:
            ctx.save_for_backward(xhat, u_in, t3, u_out, z, t, t3m)
        else:
            ctx.save_for_backward(xhat, u_in, t3, u_out, z, t)
        return yhat

    @staticmethod
    def backward(ctx, gy):
        xhat, u_in, t3, u_out, z, t = ctx.saved_tensors[:6]
        b, ci, co, r1, r2, m = ctx.dims
        gy = (gy if gy.dtype == torch.complex64 else gy.to(torch.complex64)).contiguous()
        need = ctx.needs_input_grad
        dev = xhat.device
        new = lambda *sh: torch.empty(sh, dtype=torch.complex64, device=dev)
        gx = new(b, ci, m) if need[0] else None
        gu_in = new(ci, r1) if need[1] else None
        gt3 = new(r1, r2, m) if need[2] else None
        gu_out = new(co, r2) if need[3] else None
        if b and m:
            lib = _lib.get_lib()
            p = lambda v: 0 if v is None else v.data_ptr()
            if ctx.fused and gy.data_ptr() % 16 == 0:
                # one launch: gy -> gt -> gz -> gxhat per four-mode tile, the t3 gradient mode-major (transposed back by the
                # call), the two factor gradients as per-workgroup partial sums reduced in fixed order.  The kernel always
                # forms the t3 gradient, so a scratch tensor stands in when autograd does not ask for it.
                t3m = ctx.saved_tensors[6]
                with torch.cuda.device(dev):
                    nb = lib.tucker_chain_backward_fused_workspace_bytes(ctx.dims)
                    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
                    gt3_out = gt3 if gt3 is not None else new(r1, r2, m)
                    lib.tucker_chain_backward_fused(ctx.dims, xhat.data_ptr(), u_in.data_ptr(), t3m.data_ptr(), u_out.data_ptr(),
                                                    z.data_ptr(), t.data_ptr(), gy.data_ptr(), p(gx), p(gu_in),
                                                    gt3_out.data_ptr(), p(gu_out), ws.data_ptr(), nb, _stream())
                return gx, gu_in, gt3, gu_out
            with torch.cuda.device(dev):
                nb = lib.tucker_chain_workspace_bytes(ctx.dims)
                ws = torch.empty(nb, dtype=torch.uint8, device=dev)
                # the six products of the three steps, in the order their gradients are needed: gt = gy conj(U_out),
                # gU_out = sum t^H gy, gz = gt T^H, gT = z^H gt, gxhat = gz U_in^H, gU_in = sum xhat^H gz
                lib.tucker_chain_backward(ctx.dims, xhat.data_ptr(), u_in.data_ptr(), t3.data_ptr(), u_out.data_ptr(),
                                          z.data_ptr(), t.data_ptr(), gy.data_ptr(), p(gx), p(gu_in), p(gt3), p(gu_out),
                                          ws.data_ptr(), nb, _stream())
        else:
            for v in (gx, gu_in, gt3, gu_out):
                if v is not None:
                    v.zero_()
        return gx, gu_in, gt3, gu_out


def tucker_chain(xhat, u_in, t3, u_out):
    return TuckerChainFn.apply(xhat, u_in, t3, u_out)


def mode_gemm(a, b, n_modes, conj_a=False, conj_b=False, flags=0):
    return ModeGemmFn.apply(a, b, n_modes, conj_a, conj_b, flags)


class RoundF16Fn(torch.autograd.Function):
    """``t.half()`` of the reference's half / mixed precision modes (spectral_convolution.py:436-437 and the float16
    result of the inverse transform of a complex32 spectrum) with the values kept in fp32 storage: sc_round_f16.
    The cast's autograd is a cast back, i.e. the gradient passes through."""

    @staticmethod
    def forward(ctx, t):
        _require_gpu(t, "t")
        t = t.contiguous()
        out = torch.empty_like(t)
        with torch.cuda.device(t.device):
            _lib.get_lib().round_f16(t.data_ptr(), out.data_ptr(), t.numel(), _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        return g


def round_f16(t):
    return RoundF16Fn.apply(t)


def wire_pack_c32(spec, P, rows, w0):
    """complex64 spectrum (n, C, k1, *rest) -> the complex32 wire (P, n, C, rows, *rest) of the half-precision exchange,
    one 32-bit word per element (int32 storage: torch.complex32's bytes, real part in the low half).  Spectrum row r
    lands on global wire row w0 + r of the P * rows concatenation, every other row is zero; values rounded with
    sc_round_f16.  P = 1, w0 = 0, k1 = rows: a plain conversion.  No autograd (mpu.mappings.all_to_all_c32)."""
    _require_gpu(spec, "spec")
    if spec.dtype != torch.complex64 or spec.dim() < 3:
        raise TypeError(f"wire_pack_c32: a (n, C, k1, ...) complex64 tensor, got {tuple(spec.shape)} {spec.dtype}")
    spec = spec.contiguous()
    n, c, k1 = (int(v) for v in spec.shape[:3])
    rest = list(spec.shape[3:])
    wire = torch.empty((int(P), n, c, int(rows), *rest), dtype=torch.int32, device=spec.device)
    with torch.cuda.device(spec.device):
        _lib.get_lib().wire_pack_c32(spec.data_ptr(), wire.data_ptr(), n, c, k1, math.prod(rest), int(P), int(rows),
                                     int(w0), _stream())
    return wire


def wire_unpack_c32(wire, k1, w0):
    """the complex32 wire (P, n, C, rows, *rest) (int32 words) -> complex64 (n, C, k1, *rest): rows [w0, w0 + k1) of the
    P * rows concatenation.  P = 1, w0 = 0, k1 = rows: a plain conversion.  No autograd."""
    _require_gpu(wire, "wire")
    if wire.dtype != torch.int32 or wire.dim() < 4:
        raise TypeError(f"wire_unpack_c32: a (P, n, C, rows, ...) int32 tensor, got {tuple(wire.shape)} {wire.dtype}")
    wire = wire.contiguous()
    P, n, c, rows = (int(v) for v in wire.shape[:4])
    rest = list(wire.shape[4:])
    spec = torch.empty((n, c, int(k1), *rest), dtype=torch.complex64, device=wire.device)
    with torch.cuda.device(wire.device):
        _lib.get_lib().wire_unpack_c32(wire.data_ptr(), spec.data_ptr(), n, c, int(k1), math.prod(rest), P, rows,
                                       int(w0), _stream())
    return spec


class BicubicRowsFn(torch.autograd.Function):
    """Rows [out_row0, out_row0 + out_rows) of F.interpolate(mode="bicubic", align_corners=True) of a global
    (H_in, W_in) grid to (H_out, W_out) (resample.py:49-52), from x (B, C, R, W_in) = its global rows
    [src_row0, src_row0 + R): sc_bicubic_rows_forward / _backward.  The gradient covers all R rows (halo rows
    included: the caller's exchange returns them to their owners)."""

    @staticmethod
    def forward(ctx, x, in_grid, out_grid, src_row0, out_row0, out_rows):
        _require_gpu(x, "x")
        if x.dtype != torch.float32 or x.dim() != 4:
            raise TypeError(f"bicubic rows: a (B, C, rows, W) float32 tensor, got {tuple(x.shape)} {x.dtype}")
        x = x.contiguous()
        b, c, r, w_in = (int(v) for v in x.shape)
        geo = (r, w_in, int(src_row0), int(in_grid[0]), int(out_grid[0]), int(out_grid[1]), int(out_row0), int(out_rows))
        if w_in != int(in_grid[1]):
            raise ValueError(f"bicubic rows: input width {w_in} is not the grid's {in_grid[1]}")
        y = torch.empty(b, c, int(out_rows), int(out_grid[1]), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.get_lib().bicubic_rows_forward(x.data_ptr(), y.data_ptr(), b * c, *geo, _stream())
        ctx.geo, ctx.shape = geo, (b, c)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        b, c = ctx.shape
        gx = torch.empty(b, c, ctx.geo[0], ctx.geo[1], dtype=gy.dtype, device=gy.device)
        with torch.cuda.device(gy.device):
            _lib.get_lib().bicubic_rows_backward(gy.data_ptr(), gx.data_ptr(), b * c, *ctx.geo, _stream())
        return gx, None, None, None, None, None


def _legendre(which, src, tab, rows):
    """one sc_legendre_analysis / _synthesis call: src (lines, Q, mmax) complex64, tab (lmax, nlat, mmax) float32 ->
    (lines, rows, mmax) complex64.  Both pointers reach the kernel: both tensors must be on the same GPU (a host table
    would be read by the device)."""
    _require_gpu(src, "Legendre operand")
    _require_gpu(tab, "Legendre table")
    if tab.device != src.device:
        raise ValueError(f"Legendre table on {tab.device}, operand on {src.device}: move the transform with "
                         ".to(device) first")
    src = src if src.dtype == torch.complex64 else src.to(torch.complex64)
    src = src.resolve_conj().contiguous()              # autograd hands lazily conjugated gradients on
    lines, _, mmax = (int(v) for v in src.shape)
    lmax, nlat = int(tab.shape[0]), int(tab.shape[1])
    out = torch.empty((lines, int(rows), mmax), dtype=torch.complex64, device=src.device)
    with torch.cuda.device(src.device):
        getattr(_lib.get_lib(), "legendre_" + which)(torch.view_as_real(src).data_ptr(), tab.data_ptr(),
                                                     torch.view_as_real(out).data_ptr(), lines, nlat, lmax, mmax,
                                                     _stream())
    return out


def _legendre_table(tab, lmax, nlat, mmax):
    if tab.dtype != torch.float32 or tuple(tab.shape) != (lmax, nlat, mmax) or not tab.is_contiguous():
        raise ValueError(f"Legendre table: a contiguous float32 ({lmax}, {nlat}, {mmax}) tensor, got "
                         f"{tuple(tab.shape)} {tab.dtype}")
    return tab


class LegendreAnalysisFn(torch.autograd.Function):
    """c[line, l, m] = sum_k x[line, k, m] tab[l, k, m] (sc_legendre_analysis): the latitude stage of RealSHT, x the
    (lines, nlat, mmax) output of the longitude transform, tab real.  The gradient is the synthesis kernel with the SAME
    table (tab is real: no conjugation); the table gets no gradient."""

    @staticmethod
    def forward(ctx, x, tab):
        _require_gpu(x, "x")
        if x.dim() != 3 or tab.dim() != 3:
            raise ValueError(f"Legendre analysis: x (lines, nlat, mmax) and tab (lmax, nlat, mmax), got "
                             f"{tuple(x.shape)} and {tuple(tab.shape)}")
        lmax = int(tab.shape[0])
        _legendre_table(tab, lmax, int(x.shape[1]), int(x.shape[2]))
        ctx.save_for_backward(tab)
        return _legendre("analysis", x, tab, lmax)

    @staticmethod
    def backward(ctx, gc):
        tab, = ctx.saved_tensors
        return _legendre("synthesis", gc, tab, int(tab.shape[1])), None


class LegendreSynthesisFn(torch.autograd.Function):
    """x[line, k, m] = sum_l c[line, l, m] tab[l, k, m] (sc_legendre_synthesis): the latitude stage of InverseRealSHT,
    c (lines, lmax, mmax).  The gradient is the analysis kernel with the same table."""

    @staticmethod
    def forward(ctx, c, tab):
        _require_gpu(c, "c")
        if c.dim() != 3 or tab.dim() != 3:
            raise ValueError(f"Legendre synthesis: c (lines, lmax, mmax) and tab (lmax, nlat, mmax), got "
                             f"{tuple(c.shape)} and {tuple(tab.shape)}")
        nlat = int(tab.shape[1])
        _legendre_table(tab, int(c.shape[1]), nlat, int(c.shape[2]))
        ctx.save_for_backward(tab)
        return _legendre("synthesis", c, tab, nlat)

    @staticmethod
    def backward(ctx, gx):
        tab, = ctx.saved_tensors
        return _legendre("analysis", gx, tab, int(tab.shape[0])), None


# ---- spectral-derivative multiplier pass (sc_spectral_op) -------------------------------------------------------
class SpectralTables:
    """Per-axis multiplier tables of sc_spectral_op on one device: a[d], b[d] complex64 (n_tab_d, kept_d) in the plan's
    row order (fftshift order on the non-last dims, 0 .. N/2 on the last).  Built once by the caller (float64, rounded
    once to fp32); constants of the operator, they take no gradient."""

    def __init__(self, a, b):
        if len(a) != len(b) or not 1 <= len(a) <= 3:
            raise ValueError("spectral tables: one (a, b) pair per mode dim, 1 to 3 dims")
        for ta, tb in zip(a, b):
            if ta.dtype != torch.complex64 or tb.dtype != torch.complex64 or ta.dim() != 2 or ta.shape != tb.shape \
                    or not (ta.is_contiguous() and tb.is_contiguous()) or ta.device != a[0].device \
                    or tb.device != a[0].device:
                raise ValueError("spectral tables: contiguous complex64 (n_tab, kept) pairs on one device")
        self.a, self.b = list(a), list(b)
        self.kept = tuple(int(t.shape[1]) for t in a)
        self.n_tab = tuple(int(t.shape[0]) for t in a)
        self.device = a[0].device


_SPEC_TABLES = collections.OrderedDict()       # (device, key of the caller) -> SpectralTables, least recently used first
MAX_CACHED_SPEC_TABLES = 256


def get_spectral_tables(device, key, build):
    """Cached device tables, as get_plan caches plans: ``key`` names the operator (grid, L, low-pass ratio, set of
    orders), ``build()`` returns the host tables (a, b) on a miss."""
    dev = torch.device(device)
    full = (dev.type, dev.index if dev.index is not None or dev.type != "cuda" else torch.cuda.current_device(), key)
    with _PLAN_LOCK:
        tabs = _SPEC_TABLES.get(full)
        if tabs is not None:
            _SPEC_TABLES.move_to_end(full)
            return tabs
    a, b = build()
    tabs = SpectralTables([t.to(dev) for t in a], [t.to(dev) for t in b])
    with _PLAN_LOCK:
        _SPEC_TABLES[full] = tabs
        while len(_SPEC_TABLES) > MAX_CACHED_SPEC_TABLES:
            _SPEC_TABLES.popitem(last=False)
    return tabs


def _specop_chunks(terms, n_out):
    """runs of consecutive outputs [t0, t1) whose terms plus term-less outputs fit one launch"""
    per_out = [sum(1 for t in terms if t[1] == o) for o in range(n_out)]
    for o, n in enumerate(per_out):
        if n > _lib.SC_SPECOP_MAX_TERMS:
            raise ValueError(f"output {o} sums {n} terms; sc_spectral_op takes {_lib.SC_SPECOP_MAX_TERMS} per launch")
    chunks, t0, used = [], 0, 0
    for o, n in enumerate(per_out):
        slots = max(n, 1)
        if used + slots > _lib.SC_SPECOP_MAX_TERMS:
            chunks.append((t0, o))
            t0, used = o, 0
        used += slots
    chunks.append((t0, n_out))
    return chunks


def _spectral_op(xhat, tabs, terms, n_out, conj, out_major):
    """xhat (groups, n_src, *kept) complex64 -> (n_out, groups, *kept) if out_major else (groups, n_out, *kept).
    terms: tuples (src, out, coef, (table row per dim)).  Lists too long for one launch are split over the outputs; more
    than three sources (the backward of a many-output call) are summed from launches of three."""
    _require_gpu(xhat, "spectrum")
    _require_gpu(tabs.a[0], "spectral tables")
    if tabs.device != xhat.device:
        raise ValueError(f"spectral tables on {tabs.device}, spectrum on {xhat.device}")
    xhat = xhat if xhat.dtype == torch.complex64 else xhat.to(torch.complex64)
    xhat = xhat.resolve_conj().contiguous()
    groups, n_src = int(xhat.shape[0]), int(xhat.shape[1])
    kept = tuple(int(k) for k in xhat.shape[2:])
    if kept != tabs.kept:
        raise ValueError(f"spectrum {kept} against tables for {tabs.kept}")
    for src, out, _, tab in terms:
        if not (0 <= src < n_src and 0 <= out < n_out and len(tab) == len(kept)
                and all(0 <= r < n for r, n in zip(tab, tabs.n_tab))):
            raise ValueError(f"spectral op: term {(src, out, tab)} outside {n_src} sources, {n_out} outputs, "
                             f"{tabs.n_tab} table rows")
    if n_src > 3:
        total = None
        for s0 in range(0, n_src, 3):
            part = [(s - s0, o, c, t) for s, o, c, t in terms if s0 <= s < s0 + 3]
            y = _spectral_op(xhat[:, s0:s0 + 3], tabs, part, n_out, conj, out_major)
            total = y if total is None else total.add_(y)
        return total
    modes = math.prod(kept)
    shape = (n_out, groups, *kept) if out_major else (groups, n_out, *kept)
    y = torch.empty(shape, dtype=torch.complex64, device=xhat.device)
    y_gs, y_os = (modes, groups * modes) if out_major else (n_out * modes, modes)
    lib = _lib.get_lib()
    xp, yp = torch.view_as_real(xhat).data_ptr(), torch.view_as_real(y).data_ptr()
    with torch.cuda.device(xhat.device):
        for t0, t1 in _specop_chunks(terms, n_out):
            part = [(s, o - t0, c, t) for s, o, c, t in terms if t0 <= o < t1]
            lib.spectral_op(xp, yp + 8 * t0 * y_os, kept=kept, groups=groups, n_src=n_src, n_out=t1 - t0, terms=part,
                            tabs_a=[t.data_ptr() for t in tabs.a], tabs_b=[t.data_ptr() for t in tabs.b],
                            n_tab=tabs.n_tab, y_group_stride=y_gs, y_out_stride=y_os, conj=conj, stream=_stream())
    return y


class SpectralOpFn(torch.autograd.Function):
    """yhat[g, t] = sum_{j: out_j = t} coef_j 1/2 (prod_d a_d[tab_jd] + prod_d b_d[tab_jd]) xhat[g, src_j]
    (sc_spectral_op): xhat (groups, n_src, *kept) complex64 -> (groups, n_out, *kept), or (n_out, groups, *kept) with
    out_major.  The gradient is the same call with sources and outputs exchanged and the multipliers conjugated (so it
    differentiates any number of times); the tables take none."""

    @staticmethod
    def forward(ctx, xhat, tabs, terms, n_out, conj=False, out_major=False):
        ctx.tabs, ctx.terms, ctx.conj, ctx.out_major = tabs, tuple(terms), bool(conj), bool(out_major)
        ctx.n_src = int(xhat.shape[1])
        return _spectral_op(xhat, tabs, ctx.terms, int(n_out), ctx.conj, ctx.out_major)

    @staticmethod
    def backward(ctx, g):
        if ctx.out_major:
            g = g.transpose(0, 1)
        back = tuple((o, s, c, t) for s, o, c, t in ctx.terms)
        return SpectralOpFn.apply(g, ctx.tabs, back, ctx.n_src, not ctx.conj, False), None, None, None, None, None


# ---- divergence-free spectral projection (sc_helmholtz_project) --------------------------------------------------
class HelmholtzTables:
    """Per-axis tables of sc_helmholtz_project on one device: t[d] fp32 (kept_d, 2, 3) in the plan's row order, entry
    [i, s] = (kappa, keep, z) of row i for s = 0 (the mode) and s = 1 (its mirror).  ``sel[c]`` is the axis whose kappa
    component c takes.  Built once by the caller (float64, rounded once to fp32); constants of the operator."""

    def __init__(self, t, sel, eps):
        if not 2 <= len(t) <= 3 or len(sel) != len(t) or any(not 0 <= int(s) < len(t) for s in sel):
            raise ValueError("helmholtz tables: one table and one sel entry in [0, ndim) per mode dim, 2 or 3 dims")
        for x in t:
            if x.dtype != torch.float32 or x.dim() != 3 or tuple(x.shape[1:]) != (2, 3) or not x.is_contiguous() \
                    or x.device != t[0].device:
                raise ValueError("helmholtz tables: contiguous fp32 (kept, 2, 3) tables on one device")
        if not float(eps) > 0:
            raise ValueError("helmholtz tables: eps must be positive")
        self.t, self.sel, self.eps = list(t), tuple(int(s) for s in sel), float(eps)
        self.kept = tuple(int(x.shape[0]) for x in t)
        self.device = t[0].device
        self.ptrs = [x.data_ptr() for x in self.t]


_HELM_TABLES = collections.OrderedDict()       # (device, key of the caller) -> HelmholtzTables, least recently used first


def get_helmholtz_tables(device, key, build):
    """Cached device tables, as get_spectral_tables: ``key`` names the operator (grid, lengths, modes), ``build()``
    returns (host tables, sel, eps) on a miss."""
    dev = torch.device(device)
    full = (dev.type, dev.index if dev.index is not None or dev.type != "cuda" else torch.cuda.current_device(), key)
    with _PLAN_LOCK:
        tabs = _HELM_TABLES.get(full)
        if tabs is not None:
            _HELM_TABLES.move_to_end(full)
            return tabs
    t, sel, eps = build()
    tabs = HelmholtzTables([x.to(dev) for x in t], sel, eps)
    with _PLAN_LOCK:
        _HELM_TABLES[full] = tabs
        while len(_HELM_TABLES) > MAX_CACHED_SPEC_TABLES:
            _HELM_TABLES.popitem(last=False)
    return tabs


class HelmholtzProjectFn(torch.autograd.Function):
    """u (groups, ndim, *spatial) fp32 -> its projection, the same shape: ONE real forward transform onto the block
    ``tabs.kept`` (pruned where that is smaller than the half spectrum), ONE sc_helmholtz_project launch in place, ONE
    inverse transform.  The operator is its own adjoint -- the multiplier is real, symmetric in the components and even
    in k, and the kept block holds the mirror of every mode it holds -- so backward is forward on the cotangent."""

    @staticmethod
    def forward(ctx, u, tabs):
        ctx.tabs = tabs
        _require_gpu(u, "field")
        _require_gpu(tabs.t[0], "helmholtz tables")
        if tabs.device != u.device:
            raise ValueError(f"helmholtz tables on {tabs.device}, field on {u.device}")
        u = u.contiguous().float()
        spatial, kept = [int(s) for s in u.shape[2:]], tabs.kept
        groups, nc = int(u.shape[0]), int(u.shape[1])
        if nc != len(kept) or len(spatial) != len(kept):
            raise ValueError(f"field {tuple(u.shape)} against helmholtz tables for {len(kept)} components")
        # the three C-ABI calls on one plan (unscaled forward, 1/N on the way back) and one workspace: at small grids
        # the step is bound by the host's issue rate, so nothing is looked up or allocated twice
        lib = _lib.get_lib()
        plan = get_plan(u.device, spatial, kept, "backward", 0)
        modes, n = math.prod(kept), groups * nc
        with torch.cuda.device(u.device):
            ws = _ws(lib.plan_workspace_bytes(plan, n), u.device)
            xhat = torch.empty((groups, nc, *kept, 2), dtype=torch.float32, device=u.device)
            y = torch.empty_like(u)
            stream = _stream()
            lib.transform_forward(plan, _lib.SC_FWD_SCALED, u.data_ptr(), xhat.data_ptr(), n, ws.data_ptr(), stream)
            lib.helmholtz_project(xhat.data_ptr(), xhat.data_ptr(), kept=kept, groups=groups, sel=tabs.sel,
                                  eps=tabs.eps, tabs=tabs.ptrs, y_group_stride=nc * modes, y_comp_stride=modes,
                                  stream=stream)
            lib.transform_inverse(plan, _lib.SC_INV_PADDED, xhat.data_ptr(), 0, nc, y.data_ptr(), n, ws.data_ptr(),
                                  stream)
        return y

    @staticmethod
    def backward(ctx, g):
        return HelmholtzProjectFn.apply(g.contiguous(), ctx.tabs), None


# ---- banded real-space operators: finite differences and the Lp / H1 losses (sc_band_apply, sc_sobolev_sums) -------
BAND_HALF = 3                                  # half-width of every table: taps -3 .. 3


def band_table(m, periodic):
    """Cut a dense (N, N) float64 matrix to its 7 bands: t[i, o + 3] multiplies the neighbour i + o, wrapped modulo N
    on a periodic axis (each matrix entry goes into exactly ONE tap, the nearest, so extents 1, 2, 3 -- where the
    offsets alias -- come out right).  Asserts that nothing outside the band is non-zero."""
    import numpy as np
    n = m.shape[0]
    rows = np.arange(n)
    t = np.zeros((n, 2 * BAND_HALF + 1), dtype=np.float64)
    claimed = np.zeros((n, n), dtype=bool)
    for o in sorted(range(-BAND_HALF, BAND_HALF + 1), key=abs):
        cols = rows + o
        inside = np.ones(n, dtype=bool) if periodic else (cols >= 0) & (cols < n)
        cols = cols % n
        take = inside & ~claimed[rows, cols]
        t[take, o + BAND_HALF] = m[rows[take], cols[take]]
        claimed[rows[take], cols[take]] = True
    assert not np.any(m[~claimed]), "finite-difference matrix has an entry outside its 7 bands"
    return t


def fd_matrix(n, h, order, periodic):
    """The dense float64 (N, N) matrix of FiniteDiff's derivative of `order` 1 or 2 along one axis
    (neuralop/losses/differentiation.py:328-373): central differences inside (through the wrap on a periodic axis),
    third-order one-sided rows of four entries at the two ends otherwise."""
    import numpy as np
    if order not in (1, 2):
        raise ValueError("Only 1st and 2nd order derivatives currently supported")
    if not periodic and n < 4:
        raise ValueError(f"FiniteDiff: a non-periodic axis needs at least 4 points for its one-sided boundary "
                         f"stencils, got {n}")
    m = np.zeros((n, n), dtype=np.float64)
    rows = np.arange(n)
    inner, lo, hi = ((-1.0, 0.0, 1.0), (-11.0, 18.0, -9.0, 2.0), (-2.0, 9.0, -18.0, 11.0)) if order == 1 else \
        ((1.0, -2.0, 1.0), (2.0, -5.0, 4.0, -1.0), (-1.0, 4.0, -5.0, 2.0))
    den = 2.0 * h if order == 1 else h ** 2
    end = 6.0 * h if order == 1 else h ** 2
    sel = rows if periodic else rows[1:-1]
    for o, c in zip((-1, 0, 1), inner):
        np.add.at(m, (sel, (sel + o) % n), c / den)
    if not periodic:
        m[0, :4] = np.array(lo) / end
        m[-1, -4:] = np.array(hi) / end
    return m


class BandTables:
    """Per-axis banded tables of sc_band_apply on one device: t[d] fp32 (n_tab_d, dims_d, 7); adj[d][r] is the row of
    axis d that holds the TRANSPOSE of row r (the backward pass of a term).  Built once in float64 and rounded once;
    constants of the operator, they take no gradient."""

    def __init__(self, t, periodic, adj):
        if not 1 <= len(t) <= 3 or len(periodic) != len(t) or len(adj) != len(t):
            raise ValueError("band tables: one table per axis, 1 to 3 axes")
        for ta, ad in zip(t, adj):
            if ta.dtype != torch.float32 or ta.dim() != 3 or ta.shape[2] != 2 * BAND_HALF + 1 or not ta.is_contiguous() \
                    or ta.device != t[0].device or len(ad) != ta.shape[0]:
                raise ValueError("band tables: contiguous fp32 (n_tab, extent, 7) on one device")
        self.t, self.periodic, self.adj = list(t), tuple(bool(p) for p in periodic), [tuple(a) for a in adj]
        self.dims = tuple(int(x.shape[1]) for x in t)
        self.n_tab = tuple(int(x.shape[0]) for x in t)
        self.device = t[0].device


_BAND_TABLES = collections.OrderedDict()       # (device, key) -> BandTables, least recently used first


def get_band_tables(device, key, build):
    """Cached device tables; ``key`` = (kind, dims, h, periodic flags, orders), ``build()`` returns on a miss the host
    tables (one float64 array (n_tab, extent, 7) per axis) and the transpose map ``adj``."""
    dev = torch.device(device)
    full = (dev.type, dev.index if dev.index is not None or dev.type != "cuda" else torch.cuda.current_device(), key)
    with _PLAN_LOCK:
        tabs = _BAND_TABLES.get(full)
        if tabs is not None:
            _BAND_TABLES.move_to_end(full)
            return tabs
    host, periodic, adj = build()
    tabs = BandTables([torch.from_numpy(t).to(torch.float32).contiguous().to(dev) for t in host], periodic, adj)
    with _PLAN_LOCK:
        _BAND_TABLES[full] = tabs
        while len(_BAND_TABLES) > MAX_CACHED_SPEC_TABLES:
            _BAND_TABLES.popitem(last=False)
    return tabs


def finite_diff_tables(device, dims, h, periodic, kind="fd"):
    """kind "fd": rows D1, D2, D1^T, D2^T of every axis (FiniteDiff and its backward); kind "h1": rows D1, D1^T D1 (the
    sums and the gradient of H1Loss).  From the dense float64 matrix of each axis, cut to 7 bands."""
    dims, h, periodic = tuple(int(n) for n in dims), tuple(float(v) for v in h), tuple(bool(p) for p in periodic)

    def build():
        host, adj = [], []
        for n, hd, per in zip(dims, h, periodic):
            d1 = fd_matrix(n, hd, 1, per)
            if kind == "fd":
                d2 = fd_matrix(n, hd, 2, per)
                mats, a = [d1, d2, d1.T, d2.T], (2, 3, 0, 1)
            else:
                mats, a = [d1, d1.T @ d1], (None, 1)
            import numpy as np
            host.append(np.stack([band_table(m, per) for m in mats]))
            adj.append(a)
        return host, periodic, adj

    return get_band_tables(device, (kind, dims, h, periodic, (1, 2)), build)


def _band_apply(u, u2, tabs, terms, n_out, out_major, scale=None, scale_mul=None):
    """u (groups, n_src, *dims) fp32 -> (n_out, groups, *dims) if out_major else (groups, n_out, *dims); terms: tuples
    (src, out, coef, axis, table row), axis -1 = identity.  One launch."""
    _require_gpu(u, "field")
    _require_gpu(tabs.t[0], "band tables")
    for other, what in ((u2, "second source"), (scale, "scale"), (scale_mul, "scale")):
        if other is not None:
            _require_gpu(other, what)
            if other.device != u.device or other.dtype != torch.float32 or not other.is_contiguous():
                raise ValueError(f"band apply: {what} must be contiguous fp32 on {u.device}")
    if tabs.device != u.device:
        raise ValueError(f"band tables on {tabs.device}, field on {u.device}")
    if u.dtype != torch.float32:
        raise ValueError("band apply: fp32 fields")
    u = u.contiguous()
    groups, n_src = int(u.shape[0]), int(u.shape[1])
    dims = tuple(int(k) for k in u.shape[2:])
    if dims != tabs.dims:
        raise ValueError(f"field {dims} against tables for {tabs.dims}")
    if u2 is not None and u2.shape != u.shape:
        raise ValueError(f"band apply: second source {tuple(u2.shape)} against {tuple(u.shape)}")
    if scale is not None and scale.numel() != groups or scale_mul is not None and scale_mul.numel() != 1:
        raise ValueError("band apply: scale holds one value per group, scale_mul one value")
    for src, out, _, axis, tab in terms:
        if not (0 <= src < n_src and 0 <= out < n_out and -1 <= axis < len(dims)
                and (axis < 0 or 0 <= tab < tabs.n_tab[axis])):
            raise ValueError(f"band apply: term {(src, out, axis, tab)} outside {n_src} sources, {n_out} outputs, "
                             f"{tabs.n_tab} tables")
    pts = math.prod(dims)
    y = torch.empty((n_out, groups, *dims) if out_major else (groups, n_out, *dims), dtype=torch.float32, device=u.device)
    y_gs, y_os = (pts, groups * pts) if out_major else (n_out * pts, pts)
    with torch.cuda.device(u.device):
        _lib.get_lib().band_apply(u.data_ptr(), 0 if u2 is None else u2.data_ptr(), y.data_ptr(), dims=dims,
                                  periodic=tabs.periodic, groups=groups, n_src=n_src, n_out=n_out, terms=terms,
                                  tabs=[t.data_ptr() for t in tabs.t], n_tab=tabs.n_tab, y_group_stride=y_gs,
                                  y_out_stride=y_os, scale=0 if scale is None else scale.data_ptr(),
                                  scale_mul=0 if scale_mul is None else scale_mul.data_ptr(), stream=_stream())
    return y


class BandApplyFn(torch.autograd.Function):
    """y[g, t] = sum_{j: out_j = t} coef_j M_j u[g, src_j], M_j a banded matrix along one axis or the identity
    (sc_band_apply): u (groups, n_src, *dims) fp32 -> (groups, n_out, *dims), or (n_out, groups, *dims) with out_major.
    The gradient is the same launch with sources and outputs exchanged and the transposed tables, so it differentiates
    any number of times; the tables take none."""

    @staticmethod
    def forward(ctx, u, tabs, terms, n_out, out_major=False):
        ctx.tabs, ctx.terms, ctx.out_major, ctx.n_src = tabs, tuple(terms), bool(out_major), int(u.shape[1])
        return _band_apply(u, None, tabs, ctx.terms, int(n_out), ctx.out_major)

    @staticmethod
    def backward(ctx, g):
        if ctx.out_major:
            g = g.transpose(0, 1)
        adj = ctx.tabs.adj
        back = tuple((o, s, c, a, 0 if a < 0 else adj[a][t]) for s, o, c, a, t in ctx.terms)
        if any(a >= 0 and t is None for _, _, _, a, t in back):
            raise RuntimeError("band apply: these tables carry no transpose")
        return BandApplyFn.apply(g.float().contiguous(), ctx.tabs, back, ctx.n_src, False), None, None, None, None


class SobolevSums:
    """What one forward pass of a data loss leaves behind: the reduced loss (0-dim), the per-line norms and their
    derivatives by the numerator sums (times the reduction factor)."""

    def __init__(self, loss, v, dv):
        self.loss, self.v, self.dv = loss, v, dv


def _sobolev_desc(x, y, d, **cfg):
    _require_gpu(x, "prediction")
    _require_gpu(y, "target")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f"loss: prediction {tuple(x.shape)} on {x.device} against target {tuple(y.shape)} on {y.device}")
    if x.dtype != torch.float32 or y.dtype != torch.float32 or not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("loss: contiguous fp32 operands")
    if not 1 <= d <= 3 or x.dim() < d:
        raise ValueError(f"loss: {d} spatial dims of a {x.dim()}-d tensor")
    dims = tuple(int(n) for n in x.shape[x.dim() - d:])
    lines = math.prod(int(n) for n in x.shape[:x.dim() - d])
    tabs = cfg.pop("tabs", None)
    if tabs is not None:
        _require_gpu(tabs.t[0], "band tables")
        if tabs.device != x.device or tabs.dims != dims:
            raise ValueError(f"loss: tables for {tabs.dims} on {tabs.device}, field {dims} on {x.device}")
        cfg["tabs"] = [t.data_ptr() for t in tabs.t]                  # row 0 of every axis: D
        cfg["periodic"] = tabs.periodic
    return _lib.ScEngineLib.sobolev_desc(dims=dims, lines=lines, **cfg), lines


def sobolev_sums(x, y, d, **cfg):
    """x, y (..., *dims) fp32 -> SobolevSums: stage 1 (partial sums per line and chunk) and stage 2 (the per-line norm,
    its derivative, the reduced scalar) of LpLoss / H1Loss, two launches.  cfg: h1, p, relative, take_root, reduce_mean,
    konst, eps, tabs (BandTables of kind "h1"), chunks."""
    desc, lines = _sobolev_desc(x, y, d, **cfg)
    lib = _lib.get_lib()
    nbytes = lib.sobolev_workspace_bytes(desc)
    if lines and not nbytes:
        lib.sobolev_sums(desc, x.data_ptr(), y.data_ptr(), 0, 0, 0, 0, 0)          # raises with the engine's reason
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x.device)
    out = torch.empty(2 * lines + 1, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        lib.sobolev_sums(desc, x.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes, out.data_ptr() + 4,
                         out.data_ptr() + 4 * (1 + lines), out.data_ptr(), stream=_stream())
    return SobolevSums(out[0], out[1:1 + lines], out[1 + lines:])


def lp_grad(x, y, d, dv, gout, p):
    """gx = dv[line] gout p |x - y|^(p-1) sign(x - y), shaped like x: one launch"""
    desc, lines = _sobolev_desc(x, y, d, h1=False, p=p)
    for t, what in ((dv, "dv"), (gout, "grad_output")):
        _require_gpu(t, what)
        if t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous():
            raise ValueError(f"lp_grad: {what} must be contiguous fp32 on {x.device}")
    if dv.numel() != lines or gout.numel() != 1:
        raise ValueError("lp_grad: one dv per line, one grad_output")
    gx = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.get_lib().lp_grad(desc, x.data_ptr(), y.data_ptr(), dv.data_ptr(), gout.data_ptr(), gx.data_ptr(),
                               stream=_stream())
    return gx


# ---------------------------------------------------------------------------------------------------------------------
# graph neural operator layer (sc_kernels_gno.h): radius search, CSR transpose, fused kernel integral, first layer by point
# ---------------------------------------------------------------------------------------------------------------------
def _gno_tensor(t, what, dtype=torch.float32, device=None):
    _require_gpu(t, what)
    if t.dtype != dtype:
        raise ValueError(f"gno: {what} must be {dtype}, got {t.dtype}")
    if device is not None and t.device != device:
        raise ValueError(f"gno: {what} on {t.device}, expected {device}")
    return t.contiguous()


RADIUS_METHODS = ("auto", "brute", "grid")
# "auto" takes the cell grid from this many pair tests on, for at least RADIUS_GRID_MIN_POINTS data points
RADIUS_GRID_MIN_PAIRS = 1 << 28
RADIUS_GRID_MIN_POINTS = 4096


def radius_route(n, m, d):
    """The route method="auto" takes for n data points, m queries in d dimensions: "brute" or "grid".  A function of
    the shape alone; both routes return the same bytes, so it decides the time and nothing else."""
    return "grid" if int(n) * int(m) >= RADIUS_GRID_MIN_PAIRS and int(n) >= RADIUS_GRID_MIN_POINTS else "brute"


def radius_search(data, queries, radius, return_norm=False, method="auto"):
    """Fixed-radius neighbours of every query among data (n, d), d = 1..3, as the reference's dict: neighbors_index
    int64 [E] (ascending per query), neighbors_row_splits int64 [m + 1], with return_norm weights fp32 [E] (squared
    distances, 1e-14 for coincident points).  Two passes (count + scan, fill); between them the host reads the edge
    count -- one 8-byte copy, where the reference's nonzero() synchronises too.  method: "brute" tests every pair,
    "grid" bins the data points into cells at least radius wide and tests the 3^d cells around a query, "auto" is
    radius_route(n, m, d); the result is the same bytes on either."""
    if method not in RADIUS_METHODS:
        raise ValueError(f"neighbor search: method must be one of {RADIUS_METHODS}, got {method!r}")
    data = _gno_tensor(data.detach(), "data")
    queries = _gno_tensor(queries.detach(), "queries", device=data.device)
    if data.dim() != 2 or queries.dim() != 2 or data.shape[1] != queries.shape[1] or not 1 <= data.shape[1] <= 3:
        raise ValueError(f"neighbor search: data {tuple(data.shape)} and queries {tuple(queries.shape)} must be "
                         "(n, d) and (m, d) with d = 1, 2 or 3")
    n, m, dev = int(data.shape[0]), int(queries.shape[0]), data.device
    lib = _lib.get_lib()
    desc = lib.radius_desc(data.shape[1], n, m, radius, return_norm)
    deg = torch.empty(m, dtype=torch.int32, device=dev)
    splits = torch.empty(m + 1, dtype=torch.int64, device=dev)
    grid = (radius_route(n, m, data.shape[1]) if method == "auto" else method) == "grid"
    with torch.cuda.device(dev):
        if grid:
            ws_bytes = lib.radius_grid_workspace_bytes(desc)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            lib.radius_grid_count(desc, data.data_ptr(), queries.data_ptr(), deg.data_ptr(), splits.data_ptr(),
                                  ws.data_ptr(), ws_bytes, stream=_stream())
        else:
            lib.radius_count(desc, data.data_ptr(), queries.data_ptr(), deg.data_ptr(), splits.data_ptr(),
                             stream=_stream())
        n_edges = int(splits[m].item())
        index = torch.empty(n_edges, dtype=torch.int64, device=dev)
        weights = torch.empty(n_edges, dtype=torch.float32, device=dev) if return_norm else None
        if grid:
            lib.radius_grid_fill(desc, data.data_ptr(), queries.data_ptr(), splits.data_ptr(), n_edges, index.data_ptr(),
                                 0 if weights is None else weights.data_ptr(), ws.data_ptr(), ws_bytes, stream=_stream())
        else:
            lib.radius_fill(desc, data.data_ptr(), queries.data_ptr(), splits.data_ptr(), n_edges, index.data_ptr(),
                            0 if weights is None else weights.data_ptr(), stream=_stream())
    out = {}
    if return_norm:
        out["weights"] = weights
    out["neighbors_index"] = index
    out["neighbors_row_splits"] = splits
    return out


class CsrGraph:
    """A neighbour graph in CSR form (rows = queries, columns = data points) and, built on first use by a backward pass
    and kept, its transpose: col_splits int64 [cols + 1], perm int32 [E] (edge ids by column, ascending), row_of_edge
    int32 [E].  Any valid CSR: the arrays may come from a caller, not from radius_search."""

    def __init__(self, splits, index, cols, n_edges=None):
        self.splits = _gno_tensor(splits, "neighbors_row_splits", torch.int64)
        # index None: segments only (segment_csr), n_edges given
        self.index = None if index is None else _gno_tensor(index, "neighbors_index", torch.int64, self.splits.device)
        if self.splits.dim() != 1 or self.splits.numel() < 1 or (index is not None and self.index.dim() != 1):
            raise ValueError("gno: neighbors_row_splits [m + 1] and neighbors_index [E] must be 1-d")
        self.rows, self.cols = self.splits.numel() - 1, int(cols)
        self.n_edges = int(n_edges) if index is None else self.index.numel()
        self.device = self.splits.device
        self._t = None

    def transpose(self):
        if self._t is None:
            lib, dev = _lib.get_lib(), self.device
            desc = lib.csr_desc(self.rows, self.cols, self.n_edges)
            nbytes = lib.csr_transpose_workspace_bytes(desc)
            ws = _ws(nbytes, dev)
            col_splits = torch.empty(self.cols + 1, dtype=torch.int64, device=dev)
            perm = torch.empty(self.n_edges, dtype=torch.int32, device=dev)
            row = torch.empty(self.n_edges, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                lib.csr_transpose(desc, self.splits.data_ptr(), self.index.data_ptr(), col_splits.data_ptr(),
                                  perm.data_ptr(), row.data_ptr(), ws.data_ptr(), nbytes, stream=_stream())
            self._t = (col_splits, perm, row)
        return self._t


def _csr_reduce(graph, K, F=None, w=None, mean=False, transposed=False):
    """K (E, c) or (b, E, c), F None, (nF, c) or (b, nF, c) -> (rows, c) or (b, rows, c), batched where K or F is.
    transposed: the segments are the graph's columns, F is read at the edge's row, mean scales by the ROW's degree."""
    dev = graph.device
    K = _gno_tensor(K, "edge values", device=dev)
    kb = K.dim() == 3
    c = int(K.shape[-1])
    fb = F is not None and F.dim() == 3
    if F is not None:
        F = _gno_tensor(F, "point values", device=dev)
    if w is not None:
        w = _gno_tensor(w, "edge weights", device=dev)
        if w.numel() != graph.n_edges:
            raise ValueError(f"gno: {w.numel()} edge weights for {graph.n_edges} edges")
    batch = int(K.shape[0]) if kb else (int(F.shape[0]) if fb else 1)
    if K.shape[-2] != graph.n_edges or (kb and fb and K.shape[0] != F.shape[0]) or (F is not None and F.shape[-1] != c):
        raise ValueError(f"gno: edge values {tuple(K.shape)} against {graph.n_edges} edges"
                         + ("" if F is None else f" and point values {tuple(F.shape)}"))
    if transposed:
        col_splits, perm, row = graph.transpose()
        rows, splits = graph.cols, col_splits
        kw = dict(perm=perm.data_ptr(), gather32=row.data_ptr(), n_scale_rows=graph.rows,
                  scale_splits=graph.splits.data_ptr() if mean else 0)
        need = graph.rows
    else:
        rows, splits = graph.rows, graph.splits
        kw = dict(gather64=graph.index.data_ptr() if F is not None else 0, mean=mean)
        need = graph.cols
    if F is not None and F.shape[-2] != need:
        raise ValueError(f"gno: point values {tuple(F.shape)} against {need} points")
    lib = _lib.get_lib()
    desc = lib.csr_reduce_desc(rows=rows, n_edges=graph.n_edges, channels=c, splits=splits.data_ptr(), batch=batch,
                               n_f=0 if F is None else need, k_batch_stride=graph.n_edges * c if kb else 0,
                               f_batch_stride=need * c if fb else 0, w=0 if w is None else w.data_ptr(), **kw)
    out = torch.empty((batch, rows, c) if (kb or fb) else (rows, c), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.csr_reduce(desc, K.data_ptr(), 0 if F is None else F.data_ptr(), out.data_ptr(), stream=_stream())
    return out


def _csr_edge_grad(graph, g, F, w, mean, k_batched):
    """gK (E, c), or (b, E, c) with k_batched, from g (rows, c) / (b, rows, c) and F None / (n, c) / (b, n, c)"""
    dev = graph.device
    g = _gno_tensor(g, "output gradient", device=dev)
    gb = g.dim() == 3
    batch, c = (int(g.shape[0]) if gb else 1), int(g.shape[-1])
    fb = F is not None and F.dim() == 3
    if F is not None:
        F = _gno_tensor(F, "point values", device=dev)
    lib = _lib.get_lib()
    desc = lib.csr_reduce_desc(rows=graph.rows, n_edges=graph.n_edges, channels=c, splits=graph.splits.data_ptr(),
                               batch=batch, mean=mean, n_f=0 if F is None else graph.cols,
                               k_batch_stride=graph.n_edges * c if k_batched else 0,
                               f_batch_stride=graph.cols * c if fb else 0,
                               gather64=graph.index.data_ptr() if F is not None else 0, w=0 if w is None else w.data_ptr())
    gK = torch.empty((batch, graph.n_edges, c) if k_batched else (graph.n_edges, c), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.csr_edge_grad(desc, g.data_ptr(), 0 if F is None else F.data_ptr(), gK.data_ptr(), stream=_stream())
    return gK


class KernelIntegralFn(torch.autograd.Function):
    """out[b, i] = s_i sum_{e in row i} K[(b,) e] F[b, index[e]] w[e] (sc_csr_reduce): the gather, the two products
    and the segment reduction of the reference's IntegralTransform in one launch.  Backward: gK is one sc_csr_edge_grad,
    gF one sc_csr_reduce over the transposed graph.  The weights take no gradient."""

    @staticmethod
    def forward(ctx, K, F, graph, w, mean):
        ctx.graph, ctx.mean, ctx.w = graph, bool(mean), w
        ctx.k_batched = K.dim() == 3
        ctx.f_shape = None if F is None else tuple(F.shape)
        ctx.save_for_backward(K, F)
        return _csr_reduce(graph, K, F, w, mean)

    @staticmethod
    def backward(ctx, g):
        K, F = ctx.saved_tensors
        g = g.float().contiguous()
        gK = gF = None
        if ctx.needs_input_grad[0]:
            gK = _csr_edge_grad(ctx.graph, g, F, ctx.w, ctx.mean, ctx.k_batched)
        if F is not None and ctx.needs_input_grad[1]:
            gF = _csr_reduce(ctx.graph, K, g, ctx.w, ctx.mean, transposed=True)
            if len(ctx.f_shape) == 2 and gF.dim() == 3:
                gF = gF.sum(0)
        return gK, gF, None, None, None


class EdgeLiftFn(torch.autograd.Function):
    """H[(b,) e] = act(Py[(b,) index[e]] + Px[row(e)] + bias) (sc_edge_lift): the first Linear of the kernel MLP split
    by column blocks, so that neither cat[y[idx], x_rep, f_y[idx]] nor the per-edge product is formed.  Backward:
    sc_edge_lift_bwd recomputes the pre-activation; gPy is one transposed sc_csr_reduce, gPx one row-wise one, gbias
    its column sum."""

    @staticmethod
    def forward(ctx, Py, Px, bias, graph, gelu):
        dev = graph.device
        Py, Px = _gno_tensor(Py, "Py", device=dev), _gno_tensor(Px, "Px", device=dev)
        if bias is not None:
            bias = _gno_tensor(bias, "bias", device=dev)
        c = int(Px.shape[-1])
        if Px.shape != (graph.rows, c) or Py.shape[-2:] != (graph.cols, c) or (bias is not None and bias.shape != (c,)):
            raise ValueError(f"gno: lift of Py {tuple(Py.shape)}, Px {tuple(Px.shape)} on a graph of {graph.rows} rows, "
                             f"{graph.cols} columns")
        ctx.graph, ctx.gelu = graph, bool(gelu)
        ctx.save_for_backward(Py, Px, bias)
        H = torch.empty((*Py.shape[:-2], graph.n_edges, c), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.get_lib().edge_lift(EdgeLiftFn._desc(ctx, Py), Py.data_ptr(), Px.data_ptr(),
                                     0 if bias is None else bias.data_ptr(), H.data_ptr(), stream=_stream())
        return H

    @staticmethod
    def _desc(ctx, Py):
        g, pb = ctx.graph, Py.dim() == 3
        return _lib.ScEngineLib.edge_lift_desc(
            rows=g.rows, n_edges=g.n_edges, n_py=g.cols, channels=int(Py.shape[-1]), splits=g.splits.data_ptr(),
            index=g.index.data_ptr(), batch=int(Py.shape[0]) if pb else 1,
            py_batch_stride=g.cols * int(Py.shape[-1]) if pb else 0,
            act=_lib.SC_LIFT_GELU if ctx.gelu else _lib.SC_LIFT_IDENTITY)

    @staticmethod
    def backward(ctx, gH):
        Py, Px, bias = ctx.saved_tensors
        gH = gH.float().contiguous()
        gPre = torch.empty_like(gH)
        with torch.cuda.device(gH.device):
            _lib.get_lib().edge_lift_bwd(EdgeLiftFn._desc(ctx, Py), Py.data_ptr(), Px.data_ptr(),
                                         0 if bias is None else bias.data_ptr(), gH.data_ptr(), gPre.data_ptr(),
                                         stream=_stream())
        gPy = gPx = gb = None
        if ctx.needs_input_grad[0]:
            gPy = _csr_reduce(ctx.graph, gPre, transposed=True)
        if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
            gPx = _csr_reduce(ctx.graph, gPre)
            if gPx.dim() == 3:
                gPx = gPx.sum(0)
            if bias is not None and ctx.needs_input_grad[2]:
                gb = gPx.sum(0)
        return gPy, gPx, gb, None, None


EDGE_MLP_MAX_WIDTH = _lib.SC_EDGE_MLP_MAX_WIDTH
EDGE_MLP_MAX_LAYERS = _lib.SC_EDGE_MLP_MAX_LAYERS
# kernel_route="auto" of IntegralTransform takes the fused route from this many E * b * sum(widths) on; None: never, the
# fused route is opt-in (DESIGN 3.22 has the measurements behind the choice)
EDGE_MLP_AUTO_MIN_WORK = None
# edges per chunk of the fused route, a multiple of 128; 0: the engine's default (sc_host_gno_mlp.h)
EDGE_MLP_CHUNK_EDGES = 0


def edge_mlp_route(n_edges, batch, widths):
    """The route kernel_route="auto" takes for a kernel MLP of these layer widths over n_edges edges: "edges" (one
    tensor per layer over all edges) or "fused" (EdgeMlpFn).  A function of the shape alone."""
    if EDGE_MLP_AUTO_MIN_WORK is None:
        return "edges"
    return "fused" if int(n_edges) * int(batch) * sum(int(w) for w in widths) >= EDGE_MLP_AUTO_MIN_WORK else "edges"


class EdgeMlpFn(torch.autograd.Function):
    """K[(b,) e] = the kernel MLP on gelu(Py[(b,) index[e]] + Px[row(e)] + bias0), layers 1 .. as (W_l, b_l) pairs with
    GELU between them (sc_edge_mlp_forward): one node for the whole chain, walked in chunks of edges through a workspace
    that does not grow with the edge count.  It saves its inputs alone -- point-sized tensors and parameters; backward is
    one sc_edge_mlp_backward call that recomputes each chunk.  ``calls`` counts the forward passes (tests)."""

    calls = 0

    @staticmethod
    def _desc(graph, Py, widths, chunk_edges, transposed):
        pb = Py.dim() == 3
        kw = {}
        if transposed:
            col_splits, perm, row = graph.transpose()
            kw = dict(col_splits=col_splits.data_ptr(), perm=perm.data_ptr(), row_of_edge=row.data_ptr())
        return _lib.ScEngineLib.edge_mlp_desc(
            rows=graph.rows, n_edges=graph.n_edges, n_py=graph.cols, widths=widths, splits=graph.splits.data_ptr(),
            index=graph.index.data_ptr(), batch=int(Py.shape[0]) if pb else 1,
            py_batch_stride=graph.cols * int(Py.shape[-1]) if pb else 0, chunk_edges=chunk_edges, **kw)

    @staticmethod
    def forward(ctx, Py, Px, bias0, graph, chunk_edges, *wb):
        dev = graph.device
        Py, Px = _gno_tensor(Py, "Py", device=dev), _gno_tensor(Px, "Px", device=dev)
        if bias0 is not None:
            bias0 = _gno_tensor(bias0, "bias", device=dev)
        if len(wb) % 2 or not wb:
            raise ValueError("gno: the later layers of the kernel MLP come as (weight, bias) pairs, at least one")
        Ws = [_gno_tensor(w, "weight", device=dev) for w in wb[0::2]]
        bs = [None if b is None else _gno_tensor(b, "bias", device=dev) for b in wb[1::2]]
        c = int(Px.shape[-1])
        widths = [c] + [int(w.shape[0]) for w in Ws]
        if Px.shape != (graph.rows, c) or Py.shape[-2:] != (graph.cols, c) or Py.dim() not in (2, 3) or \
                (bias0 is not None and bias0.shape != (c,)):
            raise ValueError(f"gno: kernel MLP on Py {tuple(Py.shape)}, Px {tuple(Px.shape)} and a graph of {graph.rows} "
                             f"rows, {graph.cols} columns")
        for l, (w, b) in enumerate(zip(Ws, bs)):
            if w.dim() != 2 or w.shape[1] != widths[l] or (b is not None and b.shape != (widths[l + 1],)):
                raise ValueError(f"gno: layer {l + 1} of the kernel MLP has weight {tuple(w.shape)} after {widths[l]} channels")
        ctx.graph, ctx.widths, ctx.chunk_edges = graph, widths, int(chunk_edges)
        ctx.save_for_backward(Py, Px, bias0, *Ws, *bs)
        EdgeMlpFn.calls += 1
        lib = _lib.get_lib()
        desc = EdgeMlpFn._desc(graph, Py, widths, ctx.chunk_edges, False)
        K = torch.empty((*Py.shape[:-2], graph.n_edges, widths[-1]), dtype=torch.float32, device=dev)
        nbytes = lib.edge_mlp_workspace_bytes(desc)
        if nbytes == 0:
            raise _lib.EngineError(lib.lib.sc_last_error().decode())
        ws = _ws(nbytes, dev)
        with torch.cuda.device(dev):
            lib.edge_mlp_forward(desc, Py.data_ptr(), Px.data_ptr(), 0 if bias0 is None else bias0.data_ptr(),
                                 [w.data_ptr() for w in Ws], [0 if b is None else b.data_ptr() for b in bs],
                                 K.data_ptr(), ws.data_ptr(), nbytes, stream=_stream())
        return K

    @staticmethod
    def backward(ctx, gK):
        saved = ctx.saved_tensors
        n = len(ctx.widths) - 1
        Py, Px, bias0, Ws, bs = saved[0], saved[1], saved[2], saved[3:3 + n], saved[3 + n:3 + 2 * n]
        gK = gK.float().contiguous()
        dev = gK.device
        lib = _lib.get_lib()
        desc = EdgeMlpFn._desc(ctx.graph, Py, ctx.widths, ctx.chunk_edges, ctx.graph.n_edges > 0)
        gPy, gPx = torch.empty_like(Py), torch.empty_like(Px)
        gWs = [torch.empty_like(w) for w in Ws]
        gbs = [None if b is None else torch.empty_like(b) for b in bs]
        nbytes = lib.edge_mlp_workspace_bytes(desc)
        ws = _ws(nbytes, dev)
        with torch.cuda.device(dev):
            lib.edge_mlp_backward(desc, Py.data_ptr(), Px.data_ptr(), 0 if bias0 is None else bias0.data_ptr(),
                                  [w.data_ptr() for w in Ws], [0 if b is None else b.data_ptr() for b in bs],
                                  gK.data_ptr(), gPy.data_ptr(), gPx.data_ptr(), [g.data_ptr() for g in gWs],
                                  [0 if g is None else g.data_ptr() for g in gbs], ws.data_ptr(), nbytes,
                                  stream=_stream())
        gb0 = gPx.sum(0) if bias0 is not None and ctx.needs_input_grad[2] else None
        out = [gPy, gPx, gb0, None, None]
        for gw, gb in zip(gWs, gbs):
            out += [gw, gb]
        return tuple(out)


class SegmentCsrFn(torch.autograd.Function):
    """out[(b,) i] = sum (or mean) of src[(b,) e] over row i (sc_csr_reduce with K = src)"""

    @staticmethod
    def forward(ctx, src, graph, mean):
        ctx.graph, ctx.mean, ctx.batched = graph, bool(mean), src.dim() == 3
        return _csr_reduce(graph, src, mean=mean)

    @staticmethod
    def backward(ctx, g):
        return _csr_edge_grad(ctx.graph, g.float().contiguous(), None, None, ctx.mean, ctx.batched), None, None


class EngineOps:
    """The three local stages of a (mode-parallel) spectral layer on the MI355X engine."""

    def __init__(self, fft_norm="forward", flags=0):
        self.fft_norm, self.flags = fft_norm, flags

    def forward_transform(self, x, kept, freq=None):
        return TransformForwardFn.apply(x, list(kept), self.fft_norm, self.flags, freq)

    def contract(self, xhat, w):
        return ModeContractDenseFn.apply(xhat, w)

    def inverse_transform(self, yhat, bias, spatial, freq=None, real_col=0):
        return TransformInverseFn.apply(yhat, bias, list(spatial), self.fft_norm, self.flags, freq, real_col)

    @staticmethod
    def contract_separable(xhat, w):
        """yhat[b, c, m] = xhat[b, c, m] w[c, m] (spectral_convolution.py:49-52): one 1 x 1 product per (channel, mode)"""
        b, c = int(xhat.shape[0]), int(xhat.shape[1])
        m = c
        for k in xhat.shape[2:]:
            m *= int(k)
        return mode_gemm(xhat.reshape(b, 1, m), w.reshape(1, 1, m), m).reshape(xhat.shape)

    # the latitude stage of the spherical-harmonic transforms (harmonics.RealSHT / InverseRealSHT): x (lines, nlat,
    # mmax) <-> c (lines, lmax, mmax) against a real (lmax, nlat, mmax) table
    @staticmethod
    def legendre_analysis(x, tab):
        return LegendreAnalysisFn.apply(x, tab)

    @staticmethod
    def legendre_synthesis(c, tab):
        return LegendreSynthesisFn.apply(c, tab)

    # the multiplier pass between the transforms of a spectral-derivative operator (differentiation.FourierDiff)
    @staticmethod
    def spectral_op(xhat, tabs, terms, n_out, conj=False, out_major=False):
        return SpectralOpFn.apply(xhat, tabs, terms, n_out, conj, out_major)

    # banded real-space operators (differentiation.FiniteDiff) and the reductions of losses.LpLoss / H1Loss
    @staticmethod
    def band_apply(u, tabs, terms, n_out, out_major=False):
        return BandApplyFn.apply(u, tabs, terms, n_out, out_major)

    @staticmethod
    def sobolev_sums(x, y, d, **cfg):
        return sobolev_sums(x, y, d, **cfg)

    # one complex axis of a separable transform (the sharded dim of mpu.SpatialParallelSpectralConv):
    # x (B, L, n) complex -> (B, L, k) with kept row r reading FFT index rows[r], and its zero-padded inverse;
    # 1-d complex plans with an explicit frequency map (sc_plan_desc.freq)
    def forward_axis(self, x, k, rows):
        return TransformForwardFn.apply(x, [int(k)], self.fft_norm, self.flags | SC_PLAN_COMPLEX, [list(rows)])

    def inverse_axis(self, xhat, n, rows):
        return TransformInverseFn.apply(xhat, None, [int(n)], self.fft_norm, self.flags | SC_PLAN_COMPLEX,
                                        [list(rows)], 0)

    # the 2-d skip-path resample on a row range of a global grid (mpu.SpatialParallelSpectralConv.transform): x
    # (B, C, R, W_in) holds global input rows [src_row0, src_row0 + R); returns output rows [out_row0, + out_rows)
    @staticmethod
    def interpolate_rows(x, in_grid, out_grid, src_row0, out_row0, out_rows):
        return BicubicRowsFn.apply(x, list(in_grid), list(out_grid), int(src_row0), int(out_row0), int(out_rows))


class FdConvFn(torch.autograd.Function):
    """y = (conv_pad(x, W) - conv_1x1(x, sum_taps W)) / grid_width as one folded convolution (sc_fdconv_forward);
    backward: one sc_fdconv_backward call writes gx, gW or both.  x (B, C_in, d..) fp32, weight (C_out, C_in / groups,
    k..k) fp32; padding one of periodic / zeros / replicate / reflect; grid_width a plain number."""

    @staticmethod
    def desc(x, weight, groups, padding, grid_width):
        k = int(weight.shape[-1])
        return _lib.ScEngineLib.fdconv_desc(dims=[int(s) for s in x.shape[2:]], batch=int(x.shape[0]),
                                            c_in=int(x.shape[1]), c_out=int(weight.shape[0]), k=k, groups=int(groups),
                                            padding=padding, inv_h=1.0 / float(grid_width))

    @staticmethod
    def forward(ctx, x, weight, groups, padding, grid_width):
        _require_gpu(x)
        _require_gpu(weight, "weight")
        if x.dtype != torch.float32 or weight.dtype != torch.float32:
            raise ValueError(f"fdconv: float32 tensors, got {x.dtype} and {weight.dtype}")
        nd = x.dim() - 2
        if weight.dim() != nd + 2 or x.shape[1] != weight.shape[1] * groups or len(set(weight.shape[2:])) != 1:
            raise ValueError(f"fdconv: input {tuple(x.shape)} against a weight {tuple(weight.shape)} in {groups} groups")
        x, weight = x.contiguous(), weight.contiguous()
        lib = _lib.get_lib()
        d = FdConvFn.desc(x, weight, groups, padding, grid_width)
        y = torch.empty((x.shape[0], weight.shape[0], *x.shape[2:]), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            nbytes = lib.fdconv_forward_workspace_bytes(d)
            ws = _ws(nbytes, x.device)
            lib.fdconv_forward(d, x.data_ptr(), weight.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes, stream=_stream())
        ctx.d = d
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.float().contiguous()
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_w):
            return None, None, None, None, None
        gx = torch.empty_like(x) if want_x else None
        gw = torch.empty_like(weight) if want_w else None
        with torch.cuda.device(gy.device):
            nbytes = _lib.get_lib().fdconv_workspace_bytes(ctx.d)
            ws = _ws(nbytes, gy.device)
            _lib.get_lib().fdconv_backward(ctx.d, x.data_ptr(), weight.data_ptr(), gy.data_ptr(),
                                           0 if gx is None else gx.data_ptr(), 0 if gw is None else gw.data_ptr(),
                                           ws.data_ptr(), nbytes, stream=_stream())
        return gx, gw, None, None, None


class DiscoConvFn(torch.autograd.Function):
    """The equidistant discrete-continuous convolution as one autograd node (sc_disco_forward / sc_disco_backward):
    y = conv2d(x, kernel, bias, stride, padding, groups) or, transposed, conv_transpose2d(.., output_padding) with
    kernel = q_weight sum_k psi[k] weight[.., k].  x (B, C_in, H, W), weight (.., .., K), psi (K, ph, pw) the layer's
    get_local_filter_matrix(), bias (C_out) or None, all fp32.  Saves its inputs only."""

    @staticmethod
    def desc(x, weight, psi, groups, stride, padding, output_padding, q_weight, transposed):
        c_in = int(x.shape[1])
        c_out = int(weight.shape[1]) * int(groups) if transposed else int(weight.shape[0])
        h, w, (ph, pw), (sh, sw) = int(x.shape[2]), int(x.shape[3]), psi.shape[1:], stride
        if transposed:
            out = ((h - 1) * sh - 2 * padding[0] + ph + output_padding[0],
                   (w - 1) * sw - 2 * padding[1] + pw + output_padding[1])
        else:
            out = ((h + 2 * padding[0] - ph) // sh + 1, (w + 2 * padding[1] - pw) // sw + 1)
        return _lib.ScEngineLib.disco_desc(batch=int(x.shape[0]), c_in=c_in, c_out=c_out, in_shape=(h, w),
                                           out_shape=out, basis=int(psi.shape[0]), support=(int(ph), int(pw)),
                                           stride=stride, padding=padding, output_padding=output_padding,
                                           groups=groups, q_weight=q_weight, transposed=transposed)

    @staticmethod
    def forward(ctx, x, weight, bias, psi, groups, stride, padding, output_padding, q_weight, transposed):
        _require_gpu(x)
        _require_gpu(weight, "weight")
        tensors = [x, weight, psi] + ([] if bias is None else [bias])
        if any(t.dtype != torch.float32 for t in tensors):
            raise ValueError(f"disco: float32 tensors, got {[t.dtype for t in tensors]}")
        lead = x.shape[1] if transposed else x.shape[1] // groups
        if x.dim() != 4 or weight.dim() != 3 or psi.dim() != 3 or weight.shape[2] != psi.shape[0] or \
                weight.shape[0 if transposed else 1] != lead:
            raise ValueError(f"disco: input {tuple(x.shape)} against a weight {tuple(weight.shape)} in {groups} "
                             f"groups and a filter basis {tuple(psi.shape)}")
        x, weight, psi = x.contiguous(), weight.contiguous(), psi.contiguous()
        bias = None if bias is None else bias.contiguous()
        lib = _lib.get_lib()
        d = DiscoConvFn.desc(x, weight, psi, groups, stride, padding, output_padding, q_weight, transposed)
        y = torch.empty((x.shape[0], d.c_out, max(d.h_out, 0), max(d.w_out, 0)), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            nbytes = lib.disco_forward_workspace_bytes(d)
            ws = _ws(nbytes, x.device)
            lib.disco_forward(d, x.data_ptr(), weight.data_ptr(), psi.data_ptr(), 0 if bias is None else bias.data_ptr(),
                              y.data_ptr(), ws.data_ptr(), nbytes, stream=_stream())
        ctx.d, ctx.has_bias = d, bias is not None
        ctx.save_for_backward(x, weight, psi)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, weight, psi = ctx.saved_tensors
        gy = gy.float().contiguous()
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if not (want_x or want_w or want_b):
            return (None,) * 10
        gx = torch.empty_like(x) if want_x else None
        gw = torch.empty_like(weight) if want_w else None
        gb = torch.empty(ctx.d.c_out, dtype=torch.float32, device=gy.device) if want_b else None
        lib = _lib.get_lib()
        with torch.cuda.device(gy.device):
            nbytes = lib.disco_workspace_bytes(ctx.d)
            ws = _ws(nbytes, gy.device)
            lib.disco_backward(ctx.d, x.data_ptr(), weight.data_ptr(), psi.data_ptr(), gy.data_ptr(),
                               0 if gx is None else gx.data_ptr(), 0 if gw is None else gw.data_ptr(),
                               0 if gb is None else gb.data_ptr(), ws.data_ptr(), nbytes, stream=_stream())
        return (gx, gw, gb) + (None,) * 7


class SparseDiscoFn(torch.autograd.Function):
    """The discrete-continuous convolution on point clouds as one autograd node (sc_dsparse_forward /
    sc_dsparse_backward): out[b, o, :] = sum_{c, k} weight[o, c, k] (Psi[k] (q x[b, c])) + bias.  x (B, C_in, n_in), weight
    (C_out, C_in / groups, K), bias (C_out) or None, q (n_in), all fp32; csr and csr_t are the layer's (splits, cols, vals)
    triples of Psi by (output point, basis) rows and by input-point rows (int32, int32, fp32).  Saves Z = Psi (q x) in the
    engine's layout (n_out, B, K, C_in) for the weight gradient, as the reference's autograd saves its own.  Neither pass
    waits for the device."""

    @staticmethod
    def desc(x, weight, n_out, nnz, groups):
        return _lib.ScEngineLib.dsparse_desc(batch=int(x.shape[0]), c_in=int(x.shape[1]), c_out=int(weight.shape[0]),
                                             n_in=int(x.shape[2]), n_out=int(n_out), nnz=int(nnz),
                                             basis=int(weight.shape[2]), groups=int(groups))

    @staticmethod
    def _csr(triple, rows):
        splits, cols, vals = triple
        if splits.dtype != torch.int32 or cols.dtype != torch.int32 or vals.dtype != torch.float32:
            raise ValueError("dsparse: a CSR is int32 splits, int32 columns and float32 values")
        if splits.numel() != rows + 1 or cols.numel() != vals.numel():
            raise ValueError(f"dsparse: a CSR of {rows} rows has {rows + 1} splits and as many columns as values")
        return _lib.ScEngineLib.dsparse_csr(splits.data_ptr(), cols.data_ptr(), vals.data_ptr(), rows, vals.numel())

    @staticmethod
    def forward(ctx, x, weight, bias, q, n_out, groups, csr, csr_t):
        _require_gpu(x)
        _require_gpu(weight, "weight")
        tensors = [x, weight, q] + ([] if bias is None else [bias])
        if any(t.dtype != torch.float32 for t in tensors):
            raise ValueError(f"dsparse: float32 tensors, got {[t.dtype for t in tensors]}")
        if x.dim() != 3 or weight.dim() != 3 or x.shape[1] != weight.shape[1] * groups or q.numel() != x.shape[2]:
            raise ValueError(f"dsparse: input {tuple(x.shape)} against a weight {tuple(weight.shape)} in {groups} groups "
                             f"and {q.numel()} quadrature weights")
        x, weight, q = x.contiguous(), weight.contiguous(), q.contiguous()
        bias = None if bias is None else bias.contiguous()
        csr, csr_t = tuple(t.contiguous() for t in csr), tuple(t.contiguous() for t in csr_t)
        lib = _lib.get_lib()
        d = SparseDiscoFn.desc(x, weight, n_out, csr[2].numel(), groups)
        m = SparseDiscoFn._csr(csr, d.n_out * d.basis)
        out = torch.empty((d.batch, d.c_out, d.n_out), dtype=torch.float32, device=x.device)
        z = torch.empty((d.n_out, d.batch, d.basis, d.c_in), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            nbytes = lib.dsparse_forward_workspace_bytes(d)
            ws = _ws(nbytes, x.device)
            lib.dsparse_forward(d, m, x.data_ptr(), q.data_ptr(), weight.data_ptr(), 0 if bias is None else bias.data_ptr(),
                                out.data_ptr(), z.data_ptr(), ws.data_ptr(), nbytes, stream=_stream())
        ctx.d, ctx.has_bias = d, bias is not None
        ctx.save_for_backward(weight, q, z, *csr_t)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        weight, q, z, *csr_t = ctx.saved_tensors
        gy = gy.float().contiguous()
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if not (want_x or want_w or want_b):
            return (None,) * 8
        d = ctx.d
        gx = torch.empty((d.batch, d.c_in, d.n_in), dtype=torch.float32, device=gy.device) if want_x else None
        gw = torch.empty_like(weight) if want_w else None
        gb = torch.empty(d.c_out, dtype=torch.float32, device=gy.device) if want_b else None
        lib = _lib.get_lib()
        mt = SparseDiscoFn._csr(csr_t, d.n_in)
        with torch.cuda.device(gy.device):
            nbytes = lib.dsparse_workspace_bytes(d)
            ws = _ws(nbytes, gy.device)
            lib.dsparse_backward(d, mt, q.data_ptr(), weight.data_ptr(), z.data_ptr(), gy.data_ptr(),
                                 0 if gx is None else gx.data_ptr(), 0 if gw is None else gw.data_ptr(),
                                 0 if gb is None else gb.data_ptr(), ws.data_ptr(), nbytes, stream=_stream())
        return (gx, gw, gb) + (None,) * 5


class AttnIntegralFn(torch.autograd.Function):
    """The core of AttentionKernelIntegral (associative form) as one autograd node over sc_attn_forward /
    sc_attn_backward: u = ((R q) dots) w, dots = sum_n (R LN(k))^T LN(v).  q (B, n_qry, H D), k and v (B, n_src, H D),
    pos_src (B, n_src, rotary), pos_qry (B, n_qry, rotary), inv_freq and weights (B, n_qry) or None, all fp32.  Saves
    q, k, v and dots (B, H, D, D); the backward pass recomputes the norms and rotations.  No gradient reaches the
    positions or the weights.  Neither pass waits for the device."""

    @staticmethod
    def desc(q, k, heads, rotary, has_weights):
        return _lib.ScEngineLib.attn_desc(batch=int(k.shape[0]), n_src=int(k.shape[1]), n_qry=int(q.shape[1]),
                                          heads=int(heads), head_dim=int(k.shape[2]) // int(heads), rotary=int(rotary),
                                          has_weights=int(bool(has_weights)))

    @staticmethod
    def forward(ctx, q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, heads, rotary):
        _require_gpu(q, "q")
        _require_gpu(k, "k")
        opt = [t for t in (pos_src, pos_qry, inv_freq, weights) if t is not None]
        if any(t.dtype != torch.float32 for t in [q, k, v] + opt):
            raise ValueError(f"attn: float32 tensors, got {[t.dtype for t in [q, k, v] + opt]}")
        if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2] \
                or k.shape[2] % int(heads):
            raise ValueError(f"attn: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} in {heads} heads")
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        pos_src, pos_qry, inv_freq, weights = (None if t is None else t.contiguous()
                                               for t in (pos_src, pos_qry, inv_freq, weights))
        if not rotary:
            pos_src = pos_qry = inv_freq = None
        d = AttnIntegralFn.desc(q, k, heads, rotary, weights is not None)
        if rotary and (pos_src is None or pos_qry is None or inv_freq is None
                       or tuple(pos_src.shape) != (d.batch, d.n_src, rotary)
                       or tuple(pos_qry.shape) != (d.batch, d.n_qry, rotary)
                       or inv_freq.numel() != d.head_dim // (2 * rotary)):
            raise ValueError("attn: positions (B, n, rotary) and inv_freq of head_dim / (2 rotary) entries")
        if weights is not None and weights.numel() != d.batch * d.n_qry:
            raise ValueError("attn: weights hold one value per batch and query row")
        lib = _lib.get_lib()
        u = torch.empty_like(q)
        dots = torch.empty((d.batch, d.heads, d.head_dim, d.head_dim), dtype=torch.float32, device=q.device)
        p = lambda t: 0 if t is None else t.data_ptr()                                  # noqa: E731
        with torch.cuda.device(q.device):
            nbytes = lib.attn_workspace_bytes(d)
            if nbytes == 0:
                raise ValueError(f"attn: no engine route for this shape ({lib.lib.sc_last_error().decode()})")
            ws = _ws(nbytes, q.device)
            lib.attn_forward(d, q.data_ptr(), k.data_ptr(), v.data_ptr(), p(pos_src), p(pos_qry), p(inv_freq),
                             rot_scale, p(weights), u.data_ptr(), dots.data_ptr(), ws.data_ptr(), nbytes,
                             stream=_stream())
        ctx.d, ctx.rot_scale = d, rot_scale
        ctx.has = tuple(t is not None for t in (pos_src, pos_qry, inv_freq, weights))
        ctx.save_for_backward(q, k, v, dots, *[t for t in (pos_src, pos_qry, inv_freq, weights) if t is not None])
        return u

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gu):
        q, k, v, dots, *rest = ctx.saved_tensors
        rest = list(rest)
        pos_src, pos_qry, inv_freq, weights = (rest.pop(0) if h else None for h in ctx.has)
        want = ctx.needs_input_grad[:3]
        if not any(want):
            return (None,) * 10
        gu = gu.float().contiguous()
        gq, gk, gv = (torch.empty_like(t) if w else None for t, w in zip((q, k, v), want))
        lib = _lib.get_lib()
        p = lambda t: 0 if t is None else t.data_ptr()                                  # noqa: E731
        with torch.cuda.device(gu.device):
            nbytes = lib.attn_workspace_bytes(ctx.d)
            ws = _ws(nbytes, gu.device)
            lib.attn_backward(ctx.d, q.data_ptr(), k.data_ptr(), v.data_ptr(), p(pos_src), p(pos_qry), p(inv_freq),
                              ctx.rot_scale, p(weights), dots.data_ptr(), gu.data_ptr(), p(gq), p(gk), p(gv),
                              ws.data_ptr(), nbytes, stream=_stream())
        return (gq, gk, gv) + (None,) * 7


# ---------------------------------------------------------------------------------------------------------------------
# finite differences on a point cloud (sc_kernels_nufd.h): k nearest neighbours, weights per point, apply and adjoint
# ---------------------------------------------------------------------------------------------------------------------
NUFD_MAX_K, NUFD_MAX_DERIV, NUFD_LAMBDA = 32, 8, 1e-6


def knn_search(data, queries, k):
    """The k nearest data points (n, d) of every query (m, d), d = 1..3, 3 <= k <= min(32, n): index int64 (m, k) and
    squared distances fp32 (m, k) in ascending (d2, data index).  Brute force over LDS tiles; nothing is m x n in
    memory and nothing waits for the device."""
    data = _gno_tensor(data.detach(), "data")
    queries = _gno_tensor(queries.detach(), "queries", device=data.device)
    if data.dim() != 2 or queries.dim() != 2 or data.shape[1] != queries.shape[1] or not 1 <= data.shape[1] <= 3:
        raise ValueError(f"knn: data {tuple(data.shape)} and queries {tuple(queries.shape)} must be (n, d) and (m, d) "
                         "with d = 1, 2 or 3")
    n, m, dev = int(data.shape[0]), int(queries.shape[0]), data.device
    if not 3 <= int(k) <= min(NUFD_MAX_K, n):
        raise ValueError(f"knn: k = {k} outside 3 .. min({NUFD_MAX_K}, {n} data points)")
    lib = _lib.get_lib()
    index = torch.empty((m, int(k)), dtype=torch.int64, device=dev)
    d2 = torch.empty((m, int(k)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.knn(lib.knn_desc(data.shape[1], n, m, k), data.data_ptr(), queries.data_ptr(), index.data_ptr(),
                d2.data_ptr(), stream=_stream())
    return index, d2


class NufdStencil:
    """The finite-difference stencil of a point cloud, built once: ``indices`` int64 (N, k), ``d2`` fp32 (N, k),
    ``fd_weights`` fp32 (N, n_deriv, k), ``flag`` int32 (N) (1 = ill-posed point, all its weights 0) and the transpose
    of the stencil (col_splits, perm) the adjoint gathers over.  points (N, d) fp32 on the device, d = 1..3,
    d + 1 <= k <= 32, derivative indices in [0, d), a radius only with d <= 2.  Nothing here waits for the device."""

    def __init__(self, points, k, derivative_indices, radius=None, regularize=False):
        points = _gno_tensor(points.detach(), "points")
        if points.dim() != 2 or not 1 <= points.shape[1] <= 3:
            raise ValueError(f"nufd: points {tuple(points.shape)} must be (N, d) with d = 1, 2 or 3")
        n, d, dev = int(points.shape[0]), int(points.shape[1]), points.device
        deriv = [int(i) for i in derivative_indices]
        if not max(3, d + 1) <= int(k) <= min(NUFD_MAX_K, n):
            raise ValueError(f"nufd: k = {k} outside max(3, d + 1) .. min({NUFD_MAX_K}, N = {n})")
        if not 1 <= len(deriv) <= NUFD_MAX_DERIV or any(not 0 <= i < d for i in deriv):
            raise ValueError(f"nufd: 1 to {NUFD_MAX_DERIV} derivative indices in [0, {d}), got {deriv}")
        if radius is not None and d > 2:
            raise ValueError("nufd: a radius needs d <= 2")
        self.n, self.d, self.k, self.n_deriv, self.device = n, d, int(k), len(deriv), dev
        lib = _lib.get_lib()
        self.indices, self.d2 = knn_search(points, points, self.k)
        self.fd_weights = torch.empty((n, self.n_deriv, self.k), dtype=torch.float32, device=dev)
        self.flag = torch.empty(n, dtype=torch.int32, device=dev)
        desc = lib.nufd_desc(n=n, k=self.k, n_deriv=self.n_deriv, d=d, deriv=deriv, radius=radius,
                             lam=NUFD_LAMBDA if regularize else 0.0)
        with torch.cuda.device(dev):
            lib.nufd_weights(desc, points.data_ptr(), self.indices.data_ptr(), self.d2.data_ptr(),
                             self.fd_weights.data_ptr(), self.flag.data_ptr(), stream=_stream())
        splits = torch.arange(n + 1, dtype=torch.int64, device=dev) * self.k
        self.col_splits, self.perm, _ = CsrGraph(splits, self.indices.reshape(-1), n).transpose()

    def desc(self, batch):
        return _lib.ScEngineLib.nufd_desc(n=self.n, k=self.k, n_deriv=self.n_deriv, batch=batch)


class NufdApplyFn(torch.autograd.Function):
    """out[j, b, p] = sum_m fd_weights[p, j, m] values[b, indices[p, m]] (sc_nufd_apply) for values (B, N) fp32 and a
    NufdStencil; the backward pass is one sc_nufd_apply_adjoint, a gather over the stencil's transpose in a fixed order.
    Neither pass waits for the device."""

    @staticmethod
    def forward(ctx, values, stencil):
        _require_gpu(values, "values")
        if values.dtype != torch.float32 or values.dim() != 2 or values.shape[1] != stencil.n:
            raise ValueError(f"nufd: values must be float32 (B, {stencil.n}), got {values.dtype} {tuple(values.shape)}")
        if values.device != stencil.device:
            raise ValueError(f"nufd: values on {values.device}, the stencil on {stencil.device}")
        values = values.contiguous()
        batch = int(values.shape[0])
        out = torch.empty((stencil.n_deriv, batch, stencil.n), dtype=torch.float32, device=values.device)
        if batch and stencil.n:
            with torch.cuda.device(values.device):
                _lib.get_lib().nufd_apply(stencil.desc(batch), stencil.fd_weights.data_ptr(), stencil.indices.data_ptr(),
                                          values.data_ptr(), out.data_ptr(), stream=_stream())
        ctx.stencil = stencil
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        st = ctx.stencil
        gout = gout.float().contiguous()
        batch = int(gout.shape[1])
        gv = torch.empty((batch, st.n), dtype=torch.float32, device=gout.device)
        if batch and st.n:
            with torch.cuda.device(gout.device):
                _lib.get_lib().nufd_apply_adjoint(st.desc(batch), st.fd_weights.data_ptr(), st.col_splits.data_ptr(),
                                                  st.perm.data_ptr(), gout.data_ptr(), gv.data_ptr(), stream=_stream())
        return gv, None


class EngineRawOps:
    """The local stages of a spectral layer and their adjoints as plain calls (no autograd): what a hand-scheduled
    pipeline (mpu.ModeParallelSpectralConv: transform chunk j+1 while chunk j is on the wire) is built from.
    ``out`` = a contiguous slice of a preallocated result the call writes into (no concatenation copies of the
    0.5 GB real tensors).  Real data, unchanged grid."""

    def __init__(self, fft_norm="forward", flags=0):
        self.fft_norm, self.flags = fft_norm, flags

    def _plan(self, dev, spatial, kept):
        return get_plan(dev, spatial, kept, self.fft_norm, self.flags)

    @staticmethod
    def _out(out, shape, dev):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        if tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(shape)}")
        return out

    def fwd(self, x, kept):                                   # SC_FWD_SCALED
        _require_gpu(x)
        lib = _lib.get_lib()
        x = x.contiguous().float()
        n, c = x.shape[:2]
        plan = self._plan(x.device, list(x.shape[2:]), kept)
        with torch.cuda.device(x.device):
            ws = _ws(lib.plan_workspace_bytes(plan, n * c), x.device)
            xh = torch.empty((n, c, *kept, 2), dtype=torch.float32, device=x.device)
            lib.transform_forward(plan, _lib.SC_FWD_SCALED, x.data_ptr(), xh.data_ptr(), n * c, ws.data_ptr(), _stream())
        return torch.view_as_complex(xh)

    def fwd_adjoint(self, gxhat, spatial, out=None):          # SC_INV_ADJ_R2C
        lib = _lib.get_lib()
        g = _cview(gxhat)
        n, c = g.shape[:2]
        kept = list(g.shape[2:-1])
        plan = self._plan(g.device, list(spatial), kept)
        with torch.cuda.device(g.device):
            gx = self._out(out, (n, c, *spatial), g.device)
            ws = _ws(lib.plan_workspace_bytes(plan, n * c), g.device)
            lib.transform_inverse(plan, _lib.SC_INV_ADJ_R2C, g.data_ptr(), 0, c, gx.data_ptr(), n * c, ws.data_ptr(),
                                  _stream())
        return gx

    def inv(self, yhat, bias, spatial, out=None):             # SC_INV_PADDED (+ bias)
        lib = _lib.get_lib()
        yh = _cview(yhat)
        n, c = yh.shape[:2]
        kept = list(yh.shape[2:-1])
        plan = self._plan(yh.device, list(spatial), kept)
        with torch.cuda.device(yh.device):
            y = self._out(out, (n, c, *spatial), yh.device)
            ws = _ws(lib.plan_workspace_bytes(plan, n * c), yh.device)
            bflat = None if bias is None else bias.detach().reshape(-1).float().contiguous()
            lib.transform_inverse(plan, _lib.SC_INV_PADDED, yh.data_ptr(), 0 if bflat is None else bflat.data_ptr(), c,
                                  y.data_ptr(), n * c, ws.data_ptr(), _stream())
        return y

    def inv_adjoint(self, gy, kept, want_bias=False):         # SC_FWD_ADJ_C2R (+ bias gradient off the DC row)
        lib = _lib.get_lib()
        gy = gy.contiguous().float()
        n, c = gy.shape[:2]
        plan = self._plan(gy.device, list(gy.shape[2:]), kept)
        with torch.cuda.device(gy.device):
            ws = _ws(lib.plan_workspace_bytes(plan, n * c), gy.device)
            gh = torch.empty((n, c, *kept, 2), dtype=torch.float32, device=gy.device)
            lib.transform_forward(plan, _lib.SC_FWD_ADJ_C2R, gy.data_ptr(), gh.data_ptr(), n * c, ws.data_ptr(), _stream())
            gb = None
            if want_bias:
                gb = torch.empty(c, dtype=torch.float32, device=gy.device)
                lib.bias_grad(plan, gh.data_ptr(), n, c, gb.data_ptr(), _stream())
        return torch.view_as_complex(gh), gb

    # ---- the same four stages with the spectrum in the rank-major all-to-all layout [P][n][c][rows][rest]
    #      (include/sc_engine.h, sc_spectrum_shards): the buffer handed to / received from all_to_all_single is
    #      written / read in place, no permutation copy on either side of the collective
    def _sharded(self, lib, plan, n_images, P, rows, rest, dev):
        sh = lib.shards(P, rows, n_images * rows * rest)
        return sh, _ws(lib.plan_workspace_bytes_sharded(plan, n_images), dev)

    def fwd_sharded(self, x, kept, P, rows, out=None, mode=None):       # -> [P, n, c, rows, *kept[1:], 2] float32
        _require_gpu(x)
        lib = _lib.get_lib()
        x = x.contiguous().float()
        n, c = x.shape[:2]
        rest = 1
        for k in kept[1:]:
            rest *= int(k)
        plan = self._plan(x.device, list(x.shape[2:]), kept)
        with torch.cuda.device(x.device):
            buf = self._out(out, (P, n, c, rows, *kept[1:], 2), x.device)
            sh, ws = self._sharded(lib, plan, n * c, P, rows, rest, x.device)
            lib.transform_forward_sharded(plan, _lib.SC_FWD_SCALED if mode is None else mode, x.data_ptr(),
                                          buf.data_ptr(), n * c, sh, ws.data_ptr(), _stream())
        return buf

    def inv_adjoint_sharded(self, gy, kept, P, rows, out=None, want_bias=False):
        buf = self.fwd_sharded(gy, kept, P, rows, out=out, mode=_lib.SC_FWD_ADJ_C2R)
        gb = None
        if want_bias:
            lib = _lib.get_lib()
            n, c = gy.shape[:2]
            rest = 1
            for k in kept[1:]:
                rest *= int(k)
            plan = self._plan(gy.device, list(gy.shape[2:]), kept)
            with torch.cuda.device(gy.device):
                gb = torch.empty(c, dtype=torch.float32, device=gy.device)
                lib.bias_grad_sharded(plan, buf.data_ptr(), n, c, lib.shards(P, rows, n * c * rows * rest),
                                      gb.data_ptr(), _stream())
        return buf, gb

    def inv_sharded(self, buf, bias, spatial, k1, out=None, mode=None):   # buf [P, n, c, rows, rest.., 2] float32
        lib = _lib.get_lib()
        if buf.dtype != torch.float32 or not buf.is_contiguous():
            raise ValueError("inv_sharded: a contiguous float32 [P, n, c, rows, ..., 2] buffer is required")
        P, n, c, rows = (int(v) for v in buf.shape[:4])
        kept = [int(k1)] + [int(v) for v in buf.shape[4:-1]]
        rest = 1
        for k in kept[1:]:
            rest *= k
        plan = self._plan(buf.device, list(spatial), kept)
        with torch.cuda.device(buf.device):
            y = self._out(out, (n, c, *spatial), buf.device)
            sh, ws = self._sharded(lib, plan, n * c, P, rows, rest, buf.device)
            bflat = None if bias is None else bias.detach().reshape(-1).float().contiguous()
            lib.transform_inverse_sharded(plan, _lib.SC_INV_PADDED if mode is None else mode, buf.data_ptr(),
                                          0 if bflat is None else bflat.data_ptr(), c, y.data_ptr(), n * c, sh,
                                          ws.data_ptr(), _stream())
        return y

    def fwd_adjoint_sharded(self, buf, spatial, k1, out=None):
        return self.inv_sharded(buf, None, spatial, k1, out=out, mode=_lib.SC_INV_ADJ_R2C)

    @staticmethod
    def contract(xhat, w):
        b, ci = xhat.shape[:2]
        co = w.shape[1]
        mk = xhat[0, 0].numel()
        yhat = torch.empty((b, co, *xhat.shape[2:]), dtype=torch.complex64, device=xhat.device)
        modegemm(xhat, w, P=b, Q=co, R=ci, n_modes=mk, a_strides=(ci * mk, mk, 1), b_strides=(co * mk, mk, 1),
                 out=yhat, c_strides=(co * mk, mk, 1))
        return yhat

    @staticmethod
    def contract_bwd(xhat, w, ghat, need_x=True, need_w=True):
        return dense_contract_backward(xhat, w, ghat, need_x, need_w)


    @staticmethod
    def contract_separable(xhat, w):
        """yhat[b, c, m] = xhat[b, c, m] w[c, m] (``_contract_dense_separable``, spectral_convolution.py:49-52):
        one sc_modegemm launch with (channel, mode) as the lane index, R = Q = 1."""
        b = xhat.shape[0]
        m = w.numel()
        return _raw_mode_gemm(xhat.reshape(b, 1, m), w.reshape(1, 1, m), m, False, False).reshape(xhat.shape)

    @staticmethod
    def contract_separable_bwd(xhat, w, ghat, need_x=True, need_w=True):
        b = xhat.shape[0]
        m = w.numel()
        gx = _raw_mode_gemm(ghat.reshape(b, 1, m), w.reshape(1, 1, m), m, False, True).reshape(xhat.shape) \
            if need_x else None
        gw = _raw_mode_gemm(xhat.reshape(1, b, m), ghat.reshape(b, 1, m), m, True, False).reshape(w.shape) \
            if need_w else None
        return gx, gw

    def cp_dense(self, weights, factors):
        """Dense (Cin, Cout, modes...) block of a CP weight on the engine with autograd (SpectralConv._cp_dense)."""
        from types import SimpleNamespace
        from .spectral_conv import SpectralConv
        kept = [int(f.shape[0]) for f in factors[2:]]
        return SpectralConv._cp_dense(SpectralConv, SimpleNamespace(weights=weights, factors=list(factors)), kept)

    def tt_dense(self, cores):
        """Dense block of a tensor-train weight on the engine with autograd (SpectralConv._tt_dense)."""
        from types import SimpleNamespace
        from .spectral_conv import SpectralConv
        kept = [int(c.shape[1]) for c in cores[2:]]
        return SpectralConv._tt_dense(SimpleNamespace(factors=list(cores)), kept)

    def tucker_dense(self, core, factors):
        """Dense (Cin, Cout, modes...) block of a Tucker weight on the engine, with autograd to the core and every
        factor (the chain of sc_modegemm launches of SpectralConv._tucker_dense)."""
        from types import SimpleNamespace
        from .spectral_conv import SpectralConv
        kept = [int(f.shape[0]) for f in factors[2:]]
        t3 = SpectralConv._tucker_core_times_modes(SimpleNamespace(core=core, factors=list(factors)), kept)
        m = int(t3.shape[2])
        w1 = mode_gemm(factors[0], t3, m)
        w = mode_gemm(w1, factors[1].transpose(0, 1), m)
        return w.reshape(w.shape[0], w.shape[1], *kept)