"""ctypes binding of libsc_engine.so (C-ABI: include/sc_engine.h).

The product loads exactly one library: ``neuraloperator_amd/libsc_engine.so``, the hipcc
gfx950 build of ``csrc/sc_engine.cpp``.  If it is missing the import of the engine raises --
there is no CPU or PyTorch fallback for the hot path.
"""
import atexit
import ctypes
import os
import sys
from ctypes import (POINTER, Structure, byref, c_char_p, c_int, c_int32, c_int64, c_size_t,
                    c_void_p)

SC_MAX_DIMS = 4
SC_NORM = {"forward": 0, "backward": 1, "ortho": 2}
SC_FWD_SCALED, SC_FWD_ADJ_C2R = 0, 1
SC_INV_PADDED, SC_INV_ADJ_R2C = 0, 1
SC_PLAN_FORCE_GENERIC = 1
SC_PLAN_FFT_GEN2 = 2
SC_PLAN_NO_MDFT = 4
SC_PLAN_COMPLEX = 8
SC_PLAN_IO_BF16 = 16
SC_PLAN_NO_F2P_SMALL = 32
SC_PLAN_F2P_SMALL_ALWAYS = 64
SC_PLAN_NO_SPAN = 128
SC_PLAN_NO_MX_FFT = 256
SC_PLAN_MX_FFT_3TERM = 512
SC_PLAN_PLAIN_CACHE_POLICY = 1024
SC_FREQ_DROPPED = -(1 << 63)
SC_GEMM_FORCE_VALU = 1
SC_GEMM_STREAM_C = 2
SC_GEMM_PAIRED = 4
SC_GEMM_WIDE = 8
SC_GEMM_NO_STREAM = 16
SC_GEMM_F16 = 32
SC_GEMM_NO_SB = 64
SC_GEMM_SB_WM4 = 128
SC_GEMM_NO_FMX = 1 << 24
SC_GEMM_SB_ALT_ORDER = 1 << 25
SC_GEMM_C_WT = 1 << 26
SC_GEMM_NT_A = 1 << 27
SC_GEMM_NT_B = 1 << 28


def SC_GEMM_GRID(n):
    """flags bits 8..23 of sc_modegemm_desc: cap on the matrix-core kernel's workgroups."""
    return (int(n) & 0xffff) << 8

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libsc_engine.so")


class PlanDesc(Structure):
    _fields_ = [("ndim", c_int32), ("fft_norm", c_int32),
                ("spatial", c_int64 * SC_MAX_DIMS), ("kept", c_int64 * SC_MAX_DIMS),
                ("flags", c_int32), ("real_col", c_int32),
                ("freq", POINTER(c_int64) * SC_MAX_DIMS)]


class AdamwDesc(Structure):
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("step", c_int64),
                ("correct_bias", c_int32), ("reserved", c_int32)]


class SpectrumShards(Structure):           # sc_spectrum_shards
    _fields_ = [("n_blocks", c_int64), ("rows", c_int64), ("block_stride", c_int64)]


class ModeGemmDesc(Structure):
    _fields_ = [("P", c_int64), ("Q", c_int64), ("R", c_int64), ("n_modes", c_int64),
                ("a_sp", c_int64), ("a_sr", c_int64), ("a_sm", c_int64),
                ("b_sr", c_int64), ("b_sq", c_int64), ("b_sm", c_int64),
                ("c_sp", c_int64), ("c_sq", c_int64), ("c_sm", c_int64),
                ("conj_a", c_int32), ("conj_b", c_int32),
                ("accumulate", c_int32), ("flags", c_int32),
                ("b_idx", c_void_p), ("c_idx", c_void_p),
                ("a_sg", c_int64), ("b_sg", c_int64), ("c_sg", c_int64)]


class LayerDesc(Structure):
    _fields_ = [("batch", c_int32), ("cin", c_int32), ("cout", c_int32), ("reserved", c_int32),
                ("w_extent", c_int64 * SC_MAX_DIMS), ("w_start", c_int64 * SC_MAX_DIMS)]


class Epilogue(Structure):
    _fields_ = [("skip", c_void_p), ("preact", c_void_p), ("act", c_int32), ("reserved", c_int32)]


SC_PLX_XACT, SC_PLX_ACT, SC_PLX_PRO, SC_PLX_XGRAD = 1, 2, 4, 8     # sc_plinx_desc.flags
SC_ACT_NONE, SC_ACT_GELU, SC_ACT_GELU_DGRAD = 0, 1, 2


class TuckerDesc(Structure):
    _fields_ = [("fg", c_int64), ("rx", c_int64), ("ry", c_int64), ("mx", c_int64), ("my", c_int64)]


class TuckerChainDesc(Structure):
    _fields_ = [("batch", c_int64), ("c_in", c_int64), ("c_out", c_int64), ("r_in", c_int64), ("r_out", c_int64),
                ("n_modes", c_int64)]


class PeerExchangeDesc(Structure):
    _fields_ = [("world", c_int32), ("rank", c_int32), ("block_bytes", c_int64), ("peer_window", c_void_p * 8)]


class PlinDesc(Structure):
    _fields_ = [("batch", c_int64), ("c_in", c_int64), ("c_out", c_int64), ("spatial", c_int64)]


class PlinxDesc(Structure):                                 # sc_plinx_desc (round 6)
    _fields_ = [("batch", c_int64), ("c_in", c_int64), ("c_out", c_int64), ("spatial", c_int64), ("flags", c_int32)]


class PmlpDesc(Structure):
    _fields_ = [("batch", c_int64), ("c_in", c_int64), ("c_hid", c_int64), ("c_out", c_int64), ("spatial", c_int64),
                ("act", c_int32), ("reserved", c_int32)]


SC_SPECOP_MAX_TERMS = 12


class SpecopDesc(Structure):                                # sc_specop_desc
    _fields_ = [("ndim", c_int32), ("n_src", c_int32), ("n_out", c_int32), ("n_terms", c_int32),
                ("conj", c_int32), ("reserved", c_int32), ("kept", c_int64 * 3), ("groups", c_int64),
                ("y_group_stride", c_int64), ("y_out_stride", c_int64), ("n_tab", c_int32 * 3),
                ("term_src", c_int32 * SC_SPECOP_MAX_TERMS), ("term_out", c_int32 * SC_SPECOP_MAX_TERMS),
                ("term_tab", (c_int32 * 3) * SC_SPECOP_MAX_TERMS), ("term_coef", ctypes.c_float * SC_SPECOP_MAX_TERMS),
                ("A", c_void_p * 3), ("B", c_void_p * 3)]


class HelmholtzDesc(Structure):                             # sc_helmholtz_desc
    _fields_ = [("ndim", c_int32), ("sel", c_int32 * 3), ("eps", ctypes.c_float), ("reserved", c_int32),
                ("kept", c_int64 * 3), ("groups", c_int64), ("y_group_stride", c_int64), ("y_comp_stride", c_int64),
                ("T", c_void_p * 3)]


SC_BAND_MAX_TERMS = 12


class BandDesc(Structure):                                  # sc_band_desc
    _fields_ = [("ndim", c_int32), ("n_src", c_int32), ("n_out", c_int32), ("n_terms", c_int32),
                ("dims", c_int64 * 3), ("periodic", c_int32 * 3), ("reserved", c_int32), ("groups", c_int64),
                ("y_group_stride", c_int64), ("y_out_stride", c_int64), ("n_tab", c_int32 * 3),
                ("term_src", c_int32 * SC_BAND_MAX_TERMS), ("term_out", c_int32 * SC_BAND_MAX_TERMS),
                ("term_axis", c_int32 * SC_BAND_MAX_TERMS), ("term_tab", c_int32 * SC_BAND_MAX_TERMS),
                ("term_coef", ctypes.c_float * SC_BAND_MAX_TERMS), ("T", c_void_p * 3), ("scale", c_void_p),
                ("scale_mul", c_void_p)]


class SobolevDesc(Structure):                               # sc_sobolev_desc
    _fields_ = [("ndim", c_int32), ("h1", c_int32), ("p", c_int32), ("relative", c_int32), ("take_root", c_int32),
                ("reduce_mean", c_int32), ("chunks", c_int32), ("periodic", c_int32 * 3), ("dims", c_int64 * 3),
                ("lines", c_int64), ("konst", ctypes.c_double), ("eps", ctypes.c_double), ("T", c_void_p * 3)]


class RadiusDesc(Structure):                                # sc_radius_desc
    _fields_ = [("d", c_int32), ("return_norm", c_int32), ("n", c_int64), ("m", c_int64), ("radius", ctypes.c_double)]


class CsrDesc(Structure):                                   # sc_csr_desc
    _fields_ = [("rows", c_int64), ("cols", c_int64), ("n_edges", c_int64), ("n_splits", c_int64)]


class CsrReduceDesc(Structure):                             # sc_csr_reduce_desc
    _fields_ = [("rows", c_int64), ("n_splits", c_int64), ("n_edges", c_int64), ("n_f", c_int64),
                ("n_scale_rows", c_int64), ("k_batch_stride", c_int64), ("f_batch_stride", c_int64),
                ("channels", c_int32), ("batch", c_int32), ("mean", c_int32), ("reserved", c_int32),
                ("splits", c_void_p), ("perm", c_void_p), ("gather64", c_void_p), ("gather32", c_void_p),
                ("scale_splits", c_void_p), ("w", c_void_p)]


class EdgeLiftDesc(Structure):                              # sc_edge_lift_desc
    _fields_ = [("rows", c_int64), ("n_splits", c_int64), ("n_edges", c_int64), ("n_py", c_int64),
                ("py_batch_stride", c_int64), ("channels", c_int32), ("batch", c_int32), ("act", c_int32),
                ("reserved", c_int32), ("splits", c_void_p), ("index", c_void_p)]


SC_LIFT_IDENTITY, SC_LIFT_GELU = 0, 1

SC_EDGE_MLP_MAX_LAYERS, SC_EDGE_MLP_MAX_WIDTH, SC_EDGE_MLP_TILE = 8, 512, 128


class EdgeMlpDesc(Structure):                               # sc_edge_mlp_desc
    _fields_ = [("rows", c_int64), ("n_splits", c_int64), ("n_edges", c_int64), ("n_py", c_int64),
                ("py_batch_stride", c_int64), ("chunk_edges", c_int64), ("batch", c_int32), ("n_layers", c_int32),
                ("widths", c_int32 * SC_EDGE_MLP_MAX_LAYERS), ("splits", c_void_p), ("index", c_void_p),
                ("row_of_edge", c_void_p), ("col_splits", c_void_p), ("perm", c_void_p)]


class FdconvDesc(Structure):                                # sc_fdconv_desc
    _fields_ = [("ndim", c_int32), ("k", c_int32), ("padding", c_int32), ("groups", c_int32), ("dims", c_int64 * 3),
                ("batch", c_int64), ("c_in", c_int64), ("c_out", c_int64), ("inv_h", ctypes.c_float),
                ("reserved", c_int32)]


SC_FDCONV_PADDING = {"periodic": 0, "zeros": 1, "replicate": 2, "reflect": 3}
SC_FDCONV_PATH_GENERAL, SC_FDCONV_PATH_MFMA = 1, 2


class DiscoDesc(Structure):                                 # sc_disco_desc
    _fields_ = [("batch", c_int64), ("c_in", c_int64), ("c_out", c_int64), ("h_in", c_int64), ("w_in", c_int64),
                ("h_out", c_int64), ("w_out", c_int64), ("groups", c_int32), ("basis", c_int32), ("ph", c_int32),
                ("pw", c_int32), ("sh", c_int32), ("sw", c_int32), ("pad_h", c_int32), ("pad_w", c_int32),
                ("opad_h", c_int32), ("opad_w", c_int32), ("transposed", c_int32), ("q_weight", ctypes.c_float)]


SC_DISCO_PATH_GENERAL, SC_DISCO_PATH_MFMA = 1, 2


class DsparseDesc(Structure):                               # sc_dsparse_desc
    _fields_ = [("batch", c_int64), ("c_in", c_int64), ("c_out", c_int64), ("n_in", c_int64), ("n_out", c_int64),
                ("nnz", c_int64), ("groups", c_int32), ("basis", c_int32)]


class DsparseCsr(Structure):                                # sc_dsparse_csr
    _fields_ = [("splits", c_void_p), ("cols", c_void_p), ("vals", c_void_p), ("rows", c_int64), ("nnz", c_int64)]


SC_DSPARSE_PATH_GENERAL, SC_DSPARSE_PATH_MFMA = 1, 2


class AttnDesc(Structure):                                  # sc_attn_desc
    _fields_ = [("batch", c_int64), ("n_src", c_int64), ("n_qry", c_int64), ("heads", c_int32), ("head_dim", c_int32),
                ("rotary", c_int32), ("has_weights", c_int32)]


SC_ATTN_PATH_VECTOR, SC_ATTN_PATH_MFMA = 1, 2


class KnnDesc(Structure):                                   # sc_knn_desc
    _fields_ = [("d", c_int32), ("k", c_int32), ("n", c_int64), ("m", c_int64)]


class NufdDesc(Structure):                                  # sc_nufd_desc
    _fields_ = [("n", c_int64), ("d", c_int32), ("k", c_int32), ("n_deriv", c_int32), ("batch", c_int32),
                ("deriv", c_int32 * 8), ("has_radius", c_int32), ("reserved", c_int32), ("radius", ctypes.c_double),
                ("lam", ctypes.c_double)]


class EngineError(RuntimeError):
    pass


_SHUTDOWN = False          # set at interpreter exit: device memory goes with the process, the HIP runtime may be gone


@atexit.register
def _mark_shutdown():
    global _SHUTDOWN
    _SHUTDOWN = True


class PlanHandle:
    """Owner of one sc_plan*.  ctypes passes ``_as_parameter_``; the plan (its device twiddle / index tables) is
    released by plan_destroy() or when the last reference goes away -- the plan cache of engine.py only drops ITS
    reference on eviction, autograd contexts that still hold the plan keep it alive."""

    def __init__(self, lib, ptr):
        self._lib, self._as_parameter_ = lib, ptr

    def destroy(self, _finalizing=sys.is_finalizing):
        # (the default argument keeps sys.is_finalizing reachable while module globals are being torn down: a
        # handle that outlives its module -- held by a script's globals -- is finalised after `sys` became None)
        ptr, self._as_parameter_ = self._as_parameter_, None
        try:
            if ptr is not None and self._lib is not None and not _SHUTDOWN and not _finalizing():
                self._lib.sc_plan_destroy(ptr)
        except Exception:                # interpreter shutdown
            pass

    def __del__(self):
        self.destroy()


class ScEngineLib:
    """Thin typed wrapper over the shared library.  Pointers are raw integers
    (``tensor.data_ptr()``); ``stream`` is a raw hipStream_t (0 = null stream)."""

    # every symbol include/sc_engine.h declares
    SYMBOLS = ["sc_plan_create", "sc_plan_destroy", "sc_plan_workspace_bytes", "sc_plan_is_fast",
               "sc_transform_forward", "sc_transform_inverse", "sc_modegemm",
               "sc_modegemm_msum", "sc_modegemm_msum_ws", "sc_modegemm_msum_workspace_bytes", "sc_modegemm_msum_path", "sc_modegemm_uses_matrix_cores", "sc_modegemm_path", "sc_modegemm_policy", "sc_bias_grad", "sc_adamw_step",
               "sc_layer_workspace_bytes", "sc_layer_forward", "sc_layer_backward",
               "sc_last_error", "sc_version", "sc_plan_kernel_name", "sc_transform_inverse_ex",
               "sc_layer_forward_ex", "sc_round_f16", "sc_pointwise_mlp_forward", "sc_pointwise_block_forward",
               "sc_pointwise_mlp_backward", "sc_pointwise_mlp_workspace_bytes", "sc_pointwise_linear_forward",
               "sc_pointwise_linear_backward", "sc_pointwise_linear_workspace_bytes", "sc_layer_backward_ex",
               "sc_pointwise_mlp_backward_ex", "sc_tucker_modes_supported", "sc_tucker_modes_path", "sc_tucker_modes_forward",
               "sc_tucker_modes_backward", "sc_tucker_modes_workspace_bytes", "sc_modegemm_pair",
               "sc_modegemm_pair_fused", "sc_modegemm_pair_path", "sc_plan_workspace_bytes_sharded", "sc_transform_forward_sharded",
               "sc_transform_inverse_sharded", "sc_bias_grad_sharded", "sc_tucker_chain_forward",
               "sc_tucker_chain_backward", "sc_tucker_chain_workspace_bytes", "sc_tucker_chain_fused_supported",
               "sc_tucker_chain_t3m_bytes", "sc_tucker_chain_forward_fused", "sc_tucker_chain_backward_fused",
               "sc_tucker_chain_backward_fused_workspace_bytes", "sc_peer_window_alloc", "sc_peer_window_open",
               "sc_peer_window_close", "sc_peer_window_free", "sc_peer_all_to_all", "sc_peer_window_control", "sc_pointwise_linear_forward_ex",
               "sc_pointwise_linear_workspace_bytes_ex", "sc_pointwise_linear_backward_ex", "sc_pointwise_block_backward",
               "sc_pointwise_block_backward_supported", "sc_bicubic_rows_forward", "sc_bicubic_rows_backward",
               "sc_wire_pack_c32", "sc_wire_unpack_c32", "sc_legendre_analysis", "sc_legendre_synthesis", "sc_spectral_op",
               "sc_helmholtz_project",
               "sc_band_apply", "sc_sobolev_workspace_bytes", "sc_sobolev_sums", "sc_lp_grad", "sc_radius_count",
               "sc_radius_fill", "sc_csr_transpose_workspace_bytes", "sc_csr_transpose", "sc_csr_reduce",
               "sc_csr_edge_grad", "sc_edge_lift", "sc_edge_lift_bwd", "sc_fdconv_path", "sc_fdconv_workspace_bytes",
               "sc_fdconv_forward_workspace_bytes",
               "sc_fdconv_forward", "sc_fdconv_backward", "sc_disco_path", "sc_disco_workspace_bytes",
               "sc_disco_forward_workspace_bytes", "sc_disco_forward", "sc_disco_backward", "sc_dsparse_path",
               "sc_dsparse_workspace_bytes", "sc_dsparse_forward_workspace_bytes", "sc_dsparse_forward",
               "sc_dsparse_backward", "sc_radius_grid_workspace_bytes", "sc_radius_grid_count",
               "sc_radius_grid_fill", "sc_edge_mlp_workspace_bytes", "sc_edge_mlp_forward", "sc_edge_mlp_backward",
               "sc_attn_path", "sc_attn_workspace_bytes", "sc_attn_forward", "sc_attn_backward", "sc_knn",
               "sc_nufd_weights", "sc_nufd_apply", "sc_nufd_apply_adjoint"]

    def __init__(self, path=DEFAULT_LIB):
        if not os.path.isfile(path):
            raise EngineError(
                f"{path} not found: the HIP engine is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                "There is no fallback path.")
        self.path = path
        self.lib = ctypes.CDLL(path)
        L = self.lib
        for s in self.SYMBOLS:
            if not hasattr(L, s):
                raise EngineError(f"{path} does not export {s}")
        L.sc_plan_create.argtypes = [POINTER(c_void_p), POINTER(PlanDesc)]
        L.sc_plan_create.restype = c_int
        L.sc_plan_destroy.argtypes = [c_void_p]
        L.sc_plan_destroy.restype = None
        L.sc_plan_workspace_bytes.argtypes = [c_void_p, c_int64]
        L.sc_plan_workspace_bytes.restype = c_size_t
        L.sc_plan_is_fast.argtypes = [c_void_p]
        L.sc_plan_is_fast.restype = c_int
        L.sc_transform_forward.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int64,
                                           c_void_p, c_void_p]
        L.sc_transform_forward.restype = c_int
        L.sc_transform_inverse.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int64,
                                           c_void_p, c_int64, c_void_p, c_void_p]
        L.sc_transform_inverse.restype = c_int
        L.sc_modegemm.argtypes = [POINTER(ModeGemmDesc), c_void_p, c_void_p, c_void_p, c_void_p]
        L.sc_modegemm.restype = c_int
        L.sc_modegemm_pair.argtypes = [POINTER(ModeGemmDesc), c_void_p, c_void_p, c_void_p,
                                       POINTER(ModeGemmDesc), c_void_p, c_void_p, c_void_p, c_void_p]
        L.sc_modegemm_pair.restype = c_int
        L.sc_modegemm_pair_fused.argtypes = [POINTER(ModeGemmDesc), POINTER(ModeGemmDesc)]
        L.sc_modegemm_pair_fused.restype = c_int
        L.sc_modegemm_pair_path.argtypes = [POINTER(ModeGemmDesc), POINTER(ModeGemmDesc)]
        L.sc_modegemm_pair_path.restype = c_int
        L.sc_modegemm_msum.argtypes = [POINTER(ModeGemmDesc), c_void_p, c_void_p, c_void_p, c_void_p]
        L.sc_modegemm_msum.restype = c_int
        L.sc_modegemm_msum_workspace_bytes.argtypes = [POINTER(ModeGemmDesc)]
        L.sc_modegemm_msum_workspace_bytes.restype = c_size_t
        L.sc_modegemm_msum_ws.argtypes = [POINTER(ModeGemmDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
        L.sc_modegemm_msum_ws.restype = c_int
        L.sc_modegemm_msum_path.argtypes = [POINTER(ModeGemmDesc)]
        L.sc_modegemm_msum_path.restype = c_int
        L.sc_modegemm_uses_matrix_cores.argtypes = [POINTER(ModeGemmDesc)]
        L.sc_modegemm_uses_matrix_cores.restype = c_int
        L.sc_modegemm_path.argtypes = [POINTER(ModeGemmDesc)]
        L.sc_modegemm_path.restype = c_int
        L.sc_modegemm_policy.argtypes = [POINTER(ModeGemmDesc)]
        L.sc_modegemm_policy.restype = c_int
        L.sc_bias_grad.argtypes = [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]
        L.sc_bias_grad.restype = c_int
        L.sc_plan_workspace_bytes_sharded.argtypes = [c_void_p, c_int64]
        L.sc_plan_workspace_bytes_sharded.restype = c_size_t
        L.sc_transform_forward_sharded.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int64,
                                                   POINTER(SpectrumShards), c_void_p, c_void_p]
        L.sc_transform_forward_sharded.restype = c_int
        L.sc_transform_inverse_sharded.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                                   POINTER(SpectrumShards), c_void_p, c_void_p]
        L.sc_transform_inverse_sharded.restype = c_int
        L.sc_bias_grad_sharded.argtypes = [c_void_p, c_void_p, c_int64, c_int64, POINTER(SpectrumShards), c_void_p,
                                           c_void_p]
        L.sc_bias_grad_sharded.restype = c_int
        L.sc_adamw_step.argtypes = [POINTER(AdamwDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                    c_int, c_void_p]
        L.sc_adamw_step.restype = c_int
        L.sc_layer_workspace_bytes.argtypes = [c_void_p, POINTER(LayerDesc)]
        L.sc_layer_workspace_bytes.restype = c_size_t
        L.sc_layer_forward.argtypes = [c_void_p, POINTER(LayerDesc)] + [c_void_p] * 7
        L.sc_layer_forward.restype = c_int
        L.sc_transform_inverse_ex.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int64, POINTER(Epilogue),
                                              c_void_p, c_int64, c_void_p, c_void_p]
        L.sc_transform_inverse_ex.restype = c_int
        L.sc_layer_forward_ex.argtypes = [c_void_p, POINTER(LayerDesc), c_void_p, c_void_p, c_void_p,
                                          POINTER(Epilogue), c_void_p, c_void_p, c_void_p, c_void_p]
        L.sc_layer_forward_ex.restype = c_int
        L.sc_layer_backward.argtypes = [c_void_p, POINTER(LayerDesc)] + [c_void_p] * 8
        L.sc_layer_backward_ex.argtypes = [c_void_p, POINTER(LayerDesc)] + [c_void_p] * 9
        L.sc_layer_backward_ex.restype = c_int
        L.sc_layer_backward.restype = c_int
        L.sc_pointwise_mlp_forward.argtypes = [POINTER(PmlpDesc)] + [c_void_p] * 9
        L.sc_pointwise_mlp_forward.restype = c_int
        L.sc_pointwise_block_forward.argtypes = [POINTER(PmlpDesc)] + [c_void_p] * 13
        L.sc_pointwise_block_forward.restype = c_int
        L.sc_pointwise_mlp_workspace_bytes.argtypes = [POINTER(PmlpDesc)]
        L.sc_pointwise_mlp_workspace_bytes.restype = c_size_t
        L.sc_pointwise_mlp_backward.argtypes = [POINTER(PmlpDesc)] + [c_void_p] * 17
        L.sc_pointwise_mlp_backward.restype = c_int
        L.sc_pointwise_mlp_backward_ex.argtypes = [POINTER(PmlpDesc)] + [c_void_p] * 18
        L.sc_pointwise_mlp_backward_ex.restype = c_int
        L.sc_pointwise_linear_forward.argtypes = [POINTER(PlinDesc)] + [c_void_p] * 5
        L.sc_pointwise_linear_forward.restype = c_int
        L.sc_pointwise_linear_workspace_bytes.argtypes = [POINTER(PlinDesc)]
        L.sc_pointwise_linear_workspace_bytes.restype = c_size_t
        L.sc_pointwise_block_backward_supported.argtypes = [POINTER(PmlpDesc)]
        L.sc_pointwise_block_backward_supported.restype = c_int
        L.sc_pointwise_block_backward.argtypes = [POINTER(PmlpDesc)] + [c_void_p] * 19
        L.sc_pointwise_block_backward.restype = c_int
        L.sc_pointwise_linear_forward_ex.argtypes = [POINTER(PlinxDesc)] + [c_void_p] * 8
        L.sc_pointwise_linear_forward_ex.restype = c_int
        L.sc_pointwise_linear_workspace_bytes_ex.argtypes = [POINTER(PlinxDesc)]
        L.sc_pointwise_linear_workspace_bytes_ex.restype = c_size_t
        L.sc_pointwise_linear_backward_ex.argtypes = [POINTER(PlinxDesc)] + [c_void_p] * 15
        L.sc_pointwise_linear_backward_ex.restype = c_int
        L.sc_pointwise_linear_backward.argtypes = [POINTER(PlinDesc)] + [c_void_p] * 9
        L.sc_pointwise_linear_backward.restype = c_int
        L.sc_tucker_modes_supported.argtypes = [POINTER(TuckerDesc)]
        L.sc_tucker_modes_supported.restype = c_int
        L.sc_tucker_modes_path.argtypes = [POINTER(TuckerDesc)]
        L.sc_tucker_modes_path.restype = c_int
        L.sc_tucker_modes_forward.argtypes = [POINTER(TuckerDesc)] + [c_void_p] * 5
        L.sc_tucker_modes_forward.restype = c_int
        L.sc_tucker_modes_workspace_bytes.argtypes = [POINTER(TuckerDesc)]
        L.sc_tucker_modes_workspace_bytes.restype = c_size_t
        L.sc_tucker_modes_backward.argtypes = [POINTER(TuckerDesc)] + [c_void_p] * 9
        L.sc_tucker_modes_backward.restype = c_int
        L.sc_tucker_chain_forward.argtypes = [POINTER(TuckerChainDesc)] + [c_void_p] * 8
        L.sc_tucker_chain_forward.restype = c_int
        L.sc_tucker_chain_workspace_bytes.argtypes = [POINTER(TuckerChainDesc)]
        L.sc_tucker_chain_workspace_bytes.restype = c_size_t
        L.sc_tucker_chain_backward.argtypes = [POINTER(TuckerChainDesc)] + [c_void_p] * 12 + [c_size_t, c_void_p]
        L.sc_tucker_chain_backward.restype = c_int
        L.sc_peer_window_alloc.argtypes = [c_size_t, POINTER(c_void_p), c_void_p]
        L.sc_peer_window_alloc.restype = c_int
        L.sc_peer_window_open.argtypes = [c_void_p, POINTER(c_void_p)]
        L.sc_peer_window_open.restype = c_int
        L.sc_peer_window_close.argtypes = [c_void_p]
        L.sc_peer_window_close.restype = c_int
        L.sc_peer_window_free.argtypes = [c_void_p]
        L.sc_peer_window_free.restype = c_int
        L.sc_peer_all_to_all.argtypes = [POINTER(PeerExchangeDesc), c_void_p, c_void_p, c_void_p]
        L.sc_peer_all_to_all.restype = c_int
        L.sc_peer_window_control.argtypes = [c_void_p, c_int64, POINTER(ctypes.c_int32)]
        L.sc_peer_window_control.restype = c_int
        L.sc_tucker_chain_fused_supported.argtypes = [POINTER(TuckerChainDesc)]
        L.sc_tucker_chain_fused_supported.restype = c_int
        L.sc_tucker_chain_t3m_bytes.argtypes = [POINTER(TuckerChainDesc)]
        L.sc_tucker_chain_t3m_bytes.restype = c_size_t
        L.sc_tucker_chain_forward_fused.argtypes = [POINTER(TuckerChainDesc)] + [c_void_p] * 9
        L.sc_tucker_chain_forward_fused.restype = c_int
        L.sc_tucker_chain_backward_fused_workspace_bytes.argtypes = [POINTER(TuckerChainDesc)]
        L.sc_tucker_chain_backward_fused_workspace_bytes.restype = c_size_t
        L.sc_tucker_chain_backward_fused.argtypes = [POINTER(TuckerChainDesc)] + [c_void_p] * 12 + [c_size_t, c_void_p]
        L.sc_tucker_chain_backward_fused.restype = c_int
        L.sc_round_f16.argtypes = [c_void_p, c_void_p, c_int64, c_void_p]
        L.sc_round_f16.restype = c_int
        for s in ("sc_bicubic_rows_forward", "sc_bicubic_rows_backward"):
            getattr(L, s).argtypes = [c_void_p, c_void_p] + [c_int64] * 9 + [c_void_p]
            getattr(L, s).restype = c_int
        for s in ("sc_legendre_analysis", "sc_legendre_synthesis"):
            getattr(L, s).argtypes = [c_void_p, c_void_p, c_void_p] + [c_int64] * 4 + [c_void_p]
            getattr(L, s).restype = c_int
        L.sc_spectral_op.argtypes = [POINTER(SpecopDesc), c_void_p, c_void_p, c_void_p]
        L.sc_spectral_op.restype = c_int
        L.sc_helmholtz_project.argtypes = [POINTER(HelmholtzDesc), c_void_p, c_void_p, c_void_p]
        L.sc_helmholtz_project.restype = c_int
        L.sc_band_apply.argtypes = [POINTER(BandDesc), c_void_p, c_void_p, c_void_p, c_void_p]
        L.sc_band_apply.restype = c_int
        L.sc_sobolev_workspace_bytes.argtypes = [POINTER(SobolevDesc)]
        L.sc_sobolev_workspace_bytes.restype = c_size_t
        L.sc_sobolev_sums.argtypes = [POINTER(SobolevDesc), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                      c_void_p, c_void_p]
        L.sc_sobolev_sums.restype = c_int
        L.sc_lp_grad.argtypes = [POINTER(SobolevDesc)] + [c_void_p] * 6
        L.sc_lp_grad.restype = c_int
        L.sc_radius_count.argtypes = [POINTER(RadiusDesc)] + [c_void_p] * 5
        L.sc_radius_fill.argtypes = [POINTER(RadiusDesc), c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
        L.sc_radius_grid_workspace_bytes.argtypes = [POINTER(RadiusDesc)]
        L.sc_radius_grid_workspace_bytes.restype = c_size_t
        L.sc_radius_grid_count.argtypes = [POINTER(RadiusDesc)] + [c_void_p] * 5 + [c_size_t, c_void_p]
        L.sc_radius_grid_count.restype = c_int
        L.sc_radius_grid_fill.argtypes = [POINTER(RadiusDesc), c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                          c_void_p, c_size_t, c_void_p]
        L.sc_radius_grid_fill.restype = c_int
        L.sc_csr_transpose_workspace_bytes.argtypes = [POINTER(CsrDesc)]
        L.sc_csr_transpose_workspace_bytes.restype = c_size_t
        L.sc_csr_transpose.argtypes = [POINTER(CsrDesc)] + [c_void_p] * 6 + [c_size_t, c_void_p]
        L.sc_csr_reduce.argtypes = [POINTER(CsrReduceDesc)] + [c_void_p] * 4
        L.sc_csr_edge_grad.argtypes = [POINTER(CsrReduceDesc)] + [c_void_p] * 4
        L.sc_edge_lift.argtypes = [POINTER(EdgeLiftDesc)] + [c_void_p] * 5
        L.sc_edge_lift_bwd.argtypes = [POINTER(EdgeLiftDesc)] + [c_void_p] * 6
        for s in ("sc_radius_count", "sc_radius_fill", "sc_csr_transpose", "sc_csr_reduce", "sc_csr_edge_grad",
                  "sc_edge_lift", "sc_edge_lift_bwd"):
            getattr(L, s).restype = c_int
        L.sc_edge_mlp_workspace_bytes.argtypes = [POINTER(EdgeMlpDesc)]
        L.sc_edge_mlp_workspace_bytes.restype = c_size_t
        L.sc_edge_mlp_forward.argtypes = [POINTER(EdgeMlpDesc)] + [c_void_p] * 7 + [c_size_t, c_void_p]
        L.sc_edge_mlp_forward.restype = c_int
        L.sc_edge_mlp_backward.argtypes = [POINTER(EdgeMlpDesc)] + [c_void_p] * 11 + [c_size_t, c_void_p]
        L.sc_edge_mlp_backward.restype = c_int
        L.sc_fdconv_path.argtypes = [POINTER(FdconvDesc)]
        L.sc_fdconv_path.restype = c_int
        L.sc_fdconv_workspace_bytes.argtypes = [POINTER(FdconvDesc)]
        L.sc_fdconv_workspace_bytes.restype = c_size_t
        L.sc_fdconv_forward_workspace_bytes.argtypes = [POINTER(FdconvDesc)]
        L.sc_fdconv_forward_workspace_bytes.restype = c_size_t
        L.sc_fdconv_forward.argtypes = [POINTER(FdconvDesc)] + [c_void_p] * 4 + [c_size_t, c_void_p]
        L.sc_fdconv_forward.restype = c_int
        L.sc_fdconv_backward.argtypes = [POINTER(FdconvDesc)] + [c_void_p] * 6 + [c_size_t, c_void_p]
        L.sc_fdconv_backward.restype = c_int
        L.sc_disco_path.argtypes = [POINTER(DiscoDesc)]
        L.sc_disco_path.restype = c_int
        L.sc_disco_workspace_bytes.argtypes = [POINTER(DiscoDesc)]
        L.sc_disco_workspace_bytes.restype = c_size_t
        L.sc_disco_forward_workspace_bytes.argtypes = [POINTER(DiscoDesc)]
        L.sc_disco_forward_workspace_bytes.restype = c_size_t
        L.sc_disco_forward.argtypes = [POINTER(DiscoDesc)] + [c_void_p] * 6 + [c_size_t, c_void_p]
        L.sc_disco_forward.restype = c_int
        L.sc_disco_backward.argtypes = [POINTER(DiscoDesc)] + [c_void_p] * 8 + [c_size_t, c_void_p]
        L.sc_disco_backward.restype = c_int
        L.sc_dsparse_path.argtypes = [POINTER(DsparseDesc)]
        L.sc_dsparse_path.restype = c_int
        L.sc_dsparse_workspace_bytes.argtypes = [POINTER(DsparseDesc)]
        L.sc_dsparse_workspace_bytes.restype = c_size_t
        L.sc_dsparse_forward_workspace_bytes.argtypes = [POINTER(DsparseDesc)]
        L.sc_dsparse_forward_workspace_bytes.restype = c_size_t
        L.sc_dsparse_forward.argtypes = [POINTER(DsparseDesc), POINTER(DsparseCsr)] + [c_void_p] * 7 + [c_size_t, c_void_p]
        L.sc_dsparse_forward.restype = c_int
        L.sc_dsparse_backward.argtypes = [POINTER(DsparseDesc), POINTER(DsparseCsr)] + [c_void_p] * 8 + \
            [c_size_t, c_void_p]
        L.sc_dsparse_backward.restype = c_int
        L.sc_attn_path.argtypes = [POINTER(AttnDesc)]
        L.sc_attn_path.restype = c_int
        L.sc_attn_workspace_bytes.argtypes = [POINTER(AttnDesc)]
        L.sc_attn_workspace_bytes.restype = c_size_t
        L.sc_attn_forward.argtypes = [POINTER(AttnDesc)] + [c_void_p] * 6 + [ctypes.c_float] + [c_void_p] * 4 + \
                                     [c_size_t, c_void_p]
        L.sc_attn_forward.restype = c_int
        L.sc_attn_backward.argtypes = [POINTER(AttnDesc)] + [c_void_p] * 6 + [ctypes.c_float] + [c_void_p] * 7 + \
                                      [c_size_t, c_void_p]
        L.sc_attn_backward.restype = c_int
        L.sc_knn.argtypes = [POINTER(KnnDesc)] + [c_void_p] * 5
        L.sc_nufd_weights.argtypes = [POINTER(NufdDesc)] + [c_void_p] * 6
        L.sc_nufd_apply.argtypes = [POINTER(NufdDesc)] + [c_void_p] * 5
        L.sc_nufd_apply_adjoint.argtypes = [POINTER(NufdDesc)] + [c_void_p] * 6
        for s in ("sc_knn", "sc_nufd_weights", "sc_nufd_apply", "sc_nufd_apply_adjoint"):
            getattr(L, s).restype = c_int
        for s in ("sc_wire_pack_c32", "sc_wire_unpack_c32"):
            getattr(L, s).argtypes = [c_void_p, c_void_p] + [c_int64] * 7 + [c_void_p]
            getattr(L, s).restype = c_int
        L.sc_last_error.restype = c_char_p
        L.sc_version.restype = c_char_p
        L.sc_plan_kernel_name.argtypes = [c_void_p, c_int]
        L.sc_plan_kernel_name.restype = c_char_p

    # -- helpers -----------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise EngineError(self.lib.sc_last_error().decode())

    def version(self):
        return self.lib.sc_version().decode()

    # -- plan ---------------------------------------------------------------------------
    def plan_create(self, spatial, kept, fft_norm="forward", flags=0, freq=None, real_col=0):
        """freq: optional per-dim frequency maps (None = the default same-grid rule, an entry of None
        or SC_FREQ_DROPPED = row falls off the grid); see include/sc_engine.h and modes.py."""
        d = PlanDesc()
        d.ndim = len(spatial)
        if not 1 <= d.ndim <= SC_MAX_DIMS:
            raise EngineError(f"spatial rank {d.ndim} unsupported (1..{SC_MAX_DIMS})")
        d.fft_norm = SC_NORM[fft_norm]
        for i, (n, k) in enumerate(zip(spatial, kept)):
            d.spatial[i] = int(n)
            d.kept[i] = int(k)
        d.flags = flags
        d.real_col = int(real_col)
        keep = []                                            # host arrays must outlive the call only
        if freq is not None:
            for i, f in enumerate(freq):
                if f is None:
                    continue
                if len(f) != int(kept[i]):
                    raise EngineError(f"frequency map of dim {i} has {len(f)} entries, kept = {kept[i]}")
                arr = (c_int64 * len(f))(*[SC_FREQ_DROPPED if v is None else int(v) for v in f])
                keep.append(arr)
                d.freq[i] = ctypes.cast(arr, POINTER(c_int64))
        h = c_void_p()
        self._check(self.lib.sc_plan_create(byref(h), byref(d)))
        return PlanHandle(self.lib, h)

    def plan_destroy(self, plan):
        plan.destroy()

    def plan_workspace_bytes(self, plan, n_images):
        return int(self.lib.sc_plan_workspace_bytes(plan, n_images))

    def plan_is_fast(self, plan):
        return bool(self.lib.sc_plan_is_fast(plan))

    def plan_kernel_name(self, plan, which):
        return self.lib.sc_plan_kernel_name(plan, which).decode()

    # -- sharded spectra (mode-parallel layers): the all-to-all buffer [n_blocks][n_images][rows][rest] in place
    def plan_workspace_bytes_sharded(self, plan, n_images):
        return int(self.lib.sc_plan_workspace_bytes_sharded(plan, n_images))

    @staticmethod
    def shards(n_blocks, rows, block_stride):
        return SpectrumShards(int(n_blocks), int(rows), int(block_stride))

    def transform_forward_sharded(self, plan, mode, x_ptr, xhat_ptr, n_images, shards, ws_ptr, stream=0):
        self._check(self.lib.sc_transform_forward_sharded(plan, mode, x_ptr, xhat_ptr, n_images, byref(shards),
                                                          ws_ptr, stream))

    def transform_inverse_sharded(self, plan, mode, yhat_ptr, bias_ptr, channels, y_ptr, n_images, shards, ws_ptr,
                                  stream=0):
        self._check(self.lib.sc_transform_inverse_sharded(plan, mode, yhat_ptr, bias_ptr, channels, y_ptr, n_images,
                                                          byref(shards), ws_ptr, stream))

    def bias_grad_sharded(self, plan, ghat_ptr, batch, channels, shards, gbias_ptr, stream=0):
        self._check(self.lib.sc_bias_grad_sharded(plan, ghat_ptr, batch, channels, byref(shards), gbias_ptr, stream))

    # -- stages ------------------------------------------------------------------------
    def transform_forward(self, plan, mode, x_ptr, xhat_ptr, n_images, ws_ptr, stream=0):
        self._check(self.lib.sc_transform_forward(plan, mode, x_ptr, xhat_ptr, n_images,
                                                  ws_ptr, stream))

    def transform_inverse(self, plan, mode, yhat_ptr, bias_ptr, channels, y_ptr, n_images,
                          ws_ptr, stream=0):
        self._check(self.lib.sc_transform_inverse(plan, mode, yhat_ptr, bias_ptr, channels,
                                                  y_ptr, n_images, ws_ptr, stream))

    def modegemm(self, a_ptr, b_ptr, c_ptr, stream=0, **kw):
        self._check(self.lib.sc_modegemm(byref(self._gemm_desc(kw)), a_ptr, b_ptr, c_ptr, stream))

    _DESC_CACHE = {}

    @staticmethod
    def _gemm_desc(kw):
        """The descriptor of a contraction, cached by value: building a 22-field ctypes structure through setattr costs
        about as much host time as the launch itself (a factorized layer step issues ~20 of them)."""
        key = tuple(kw.items())
        d = ScEngineLib._DESC_CACHE.get(key)
        if d is None:
            if len(ScEngineLib._DESC_CACHE) > 4096:
                ScEngineLib._DESC_CACHE.clear()
            d = ModeGemmDesc()
            for k, v in kw.items():
                setattr(d, k, v)
            ScEngineLib._DESC_CACHE[key] = d
        return d

    def modegemm_pair(self, kw0, a0, b0, c0, kw1, a1, b1, c1, stream=0):
        """sc_modegemm(kw0 ...) and sc_modegemm(kw1 ...), one launch when the pair qualifies (a layer's backward)."""
        d0, d1 = self._gemm_desc(kw0), self._gemm_desc(kw1)
        self._check(self.lib.sc_modegemm_pair(byref(d0), a0, b0, c0, byref(d1), a1, b1, c1, stream))

    def modegemm_pair_fused(self, kw0, kw1):
        d0, d1 = self._gemm_desc(kw0), self._gemm_desc(kw1)
        return bool(self.lib.sc_modegemm_pair_fused(byref(d0), byref(d1)))

    def modegemm_pair_path(self, kw0, kw1):
        """2 = one pass over the weight (k_modegemm_sb_bwd), 1 = one k_modegemm_dma_bwd launch, 0 = two launches."""
        d0, d1 = self._gemm_desc(kw0), self._gemm_desc(kw1)
        return int(self.lib.sc_modegemm_pair_path(byref(d0), byref(d1)))

    def pointwise_mlp_forward(self, batch, c_in, c_hid, c_out, spatial, act, x, w1, b1, w2, b2, skip, gate, out, stream=0):
        d = PmlpDesc(batch, c_in, c_hid, c_out, spatial, act, 0)
        self._check(self.lib.sc_pointwise_mlp_forward(byref(d), x, w1, b1, w2, b2, skip, gate, out, stream))

    def pointwise_mlp_workspace_bytes(self, batch, c_in, c_hid, c_out, spatial, act):
        d = PmlpDesc(batch, c_in, c_hid, c_out, spatial, act, 0)
        return int(self.lib.sc_pointwise_mlp_workspace_bytes(byref(d)))

    def pointwise_block_forward(self, batch, c, c_hid, spatial, act, conv, x, ws, bs, w1, b1, w2, b2, gate, y, pre, out,
                                stream=0):
        """s = conv + (ws x + bs); y = act(s); out = act(W2 gelu(W1 y + b1) + b2 + gate x) in one pass (y, pre stored)."""
        d = PmlpDesc(batch, c, c_hid, c, spatial, act, 0)
        self._check(self.lib.sc_pointwise_block_forward(byref(d), conv, x, ws, bs, w1, b1, w2, b2, gate, y, pre, out, stream))

    def pointwise_mlp_backward(self, batch, c_in, c_hid, c_out, spatial, act, x, w1, b1, w2, b2, skip, gate, gout,
                               gx, gw1, gb1, gw2, gb2, gskip, ggate, ws, stream=0, x_pre=0):
        d = PmlpDesc(batch, c_in, c_hid, c_out, spatial, act, 0)
        self._check(self.lib.sc_pointwise_mlp_backward_ex(byref(d), x, x_pre, w1, b1, w2, b2, skip, gate, gout, gx, gw1,
                                                          gb1, gw2, gb2, gskip, ggate, ws, stream))

    def pointwise_block_backward_supported(self, batch, c, c_hid, spatial):
        return bool(self.lib.sc_pointwise_block_backward_supported(byref(PmlpDesc(batch, c, c_hid, c, spatial, 0, 0))))

    def pointwise_block_backward(self, batch, c, c_hid, spatial, act, y, y_pre, x, ws_lin, w1, b1, w2, b2, gate, gout, gz, gin,
                                 gw1, gb1, gw2, gb2, ggate, ws, stream=0):
        """the MLP pass of a block's backward + the data path of its linear skip (include/sc_engine.h, round 6)"""
        d = PmlpDesc(batch, c, c_hid, c, spatial, act, 0)
        self._check(self.lib.sc_pointwise_block_backward(byref(d), y, y_pre, x, ws_lin, w1, b1, w2, b2, gate, gout, gz, gin,
                                                         gw1, gb1, gw2, gb2, ggate, ws, stream))

    def pointwise_linear_forward(self, batch, c_in, c_out, spatial, x, w, bias, out, stream=0):
        d = PlinDesc(batch, c_in, c_out, spatial)
        self._check(self.lib.sc_pointwise_linear_forward(byref(d), x, w, bias, out, stream))

    def pointwise_linear_workspace_bytes(self, batch, c_in, c_out, spatial):
        d = PlinDesc(batch, c_in, c_out, spatial)
        return int(self.lib.sc_pointwise_linear_workspace_bytes(byref(d)))

    def pointwise_linear_backward(self, batch, c_in, c_out, spatial, x, w, gout, gx, gw, gbias, ws, stream=0, addend=0):
        d = PlinDesc(batch, c_in, c_out, spatial)
        self._check(self.lib.sc_pointwise_linear_backward(byref(d), x, w, gout, addend, gx, gw, gbias, ws, stream))

    # ---- 1 x 1 maps with the block's pointwise operations in their load / store paths (round 6; include/sc_engine.h)
    def pointwise_linear_forward_ex(self, batch, c_in, c_out, spatial, flags, x, w, bias, skip, gate, out, pre_out=0, stream=0):
        d = PlinxDesc(batch, c_in, c_out, spatial, flags)
        self._check(self.lib.sc_pointwise_linear_forward_ex(byref(d), x, w, bias, skip, gate, out, pre_out, stream))

    def pointwise_linear_workspace_bytes_ex(self, batch, c_in, c_out, spatial):
        return int(self.lib.sc_pointwise_linear_workspace_bytes_ex(byref(PlinxDesc(batch, c_in, c_out, spatial, 0))))

    def pointwise_linear_backward_ex(self, batch, c_in, c_out, spatial, flags, x, w, gout, pre, xg, skip, gate, addend, gx, gw,
                                     gbias, gskip, ggate, ws, stream=0):
        d = PlinxDesc(batch, c_in, c_out, spatial, flags)
        self._check(self.lib.sc_pointwise_linear_backward_ex(byref(d), x, w, gout, pre, xg, skip, gate, addend, gx, gw, gbias,
                                                             gskip, ggate, ws, stream))

    def tucker_modes_supported(self, fg, rx, ry, mx, my):
        return bool(self.lib.sc_tucker_modes_supported(byref(TuckerDesc(fg, rx, ry, mx, my))))

    def tucker_modes_path(self, fg, rx, ry, mx, my):
        """0: unsupported, 1: the vector kernels, else 10 f + b: forward k_tucker_modes_fwd_mx<4, 3>, <4, 4>, <16, 3>,
        <16, 4> for f = 1..4, backward k_tucker_modes_bwd_mx<3, 9, 3, 3, 2> for b = 1, <16, 16, 4, 4, 4> for b = 2."""
        return int(self.lib.sc_tucker_modes_path(byref(TuckerDesc(fg, rx, ry, mx, my))))

    def tucker_modes_forward(self, fg, rx, ry, mx, my, core, ux, uy, t, stream=0):
        self._check(self.lib.sc_tucker_modes_forward(byref(TuckerDesc(fg, rx, ry, mx, my)), core, ux, uy, t, stream))

    def tucker_modes_workspace_bytes(self, fg, rx, ry, mx, my):
        return int(self.lib.sc_tucker_modes_workspace_bytes(byref(TuckerDesc(fg, rx, ry, mx, my))))

    def tucker_modes_backward(self, fg, rx, ry, mx, my, core, ux, uy, gt, gcore, gux, guy, ws, stream=0):
        self._check(self.lib.sc_tucker_modes_backward(byref(TuckerDesc(fg, rx, ry, mx, my)), core, ux, uy, gt, gcore, gux,
                                                      guy, ws, stream))

    def tucker_chain_forward(self, dims, xhat, u_in, t3, u_out, z, t, yhat, stream=0):
        """dims = (batch, c_in, c_out, r_in, r_out, n_modes); device pointers of contiguous complex64 arrays"""
        self._check(self.lib.sc_tucker_chain_forward(byref(TuckerChainDesc(*dims)), xhat, u_in, t3, u_out, z, t, yhat, stream))

    def tucker_chain_workspace_bytes(self, dims):
        return int(self.lib.sc_tucker_chain_workspace_bytes(byref(TuckerChainDesc(*dims))))

    def tucker_chain_backward(self, dims, xhat, u_in, t3, u_out, z, t, gy, gxhat, gu_in, gt3, gu_out, ws, ws_bytes, stream=0):
        """null (0) gradient pointers skip that gradient"""
        self._check(self.lib.sc_tucker_chain_backward(byref(TuckerChainDesc(*dims)), xhat, u_in, t3, u_out, z, t, gy, gxhat,
                                                      gu_in, gt3, gu_out, ws, ws_bytes, stream))

    # ---- peer-store exchange (round 5; include/sc_engine.h)
    def peer_window_alloc(self, data_bytes):
        """-> (device pointer, 64-byte IPC handle) of a fresh fine-grained window"""
        import ctypes
        ptr, handle = c_void_p(), ctypes.create_string_buffer(64)
        self._check(self.lib.sc_peer_window_alloc(data_bytes, byref(ptr), handle))
        return int(ptr.value), handle.raw

    def peer_window_open(self, handle):
        import ctypes
        ptr, buf = c_void_p(), ctypes.create_string_buffer(bytes(handle), 64)
        self._check(self.lib.sc_peer_window_open(buf, byref(ptr)))
        return int(ptr.value)

    def peer_window_close(self, ptr):
        self._check(self.lib.sc_peer_window_close(ptr))

    def peer_window_free(self, ptr):
        self._check(self.lib.sc_peer_window_free(ptr))

    def peer_window_control(self, own_window, spin_budget_ms=-1):
        """set the spin budget of the waits on this rank's window (ms; 0 = unbounded, < 0 = unchanged); -> the error word a
        timed-out wait left (0 = none, 1 + p = peer p's flag never came), cleared by the read"""
        import ctypes
        err = ctypes.c_int32(0)
        self._check(self.lib.sc_peer_window_control(own_window, spin_budget_ms, byref(err)))
        return int(err.value)

    def peer_all_to_all(self, world, rank, block_bytes, peer_windows, send, recv, stream=0):
        d = PeerExchangeDesc(world, rank, block_bytes, (c_void_p * 8)(*(list(peer_windows) + [None] * (8 - len(peer_windows)))))
        self._check(self.lib.sc_peer_all_to_all(byref(d), send, recv, stream))

    # ---- the chain as one launch each way (round 5; include/sc_engine.h)
    def tucker_chain_fused_supported(self, dims):
        return bool(self.lib.sc_tucker_chain_fused_supported(byref(TuckerChainDesc(*dims))))

    def tucker_chain_t3m_bytes(self, dims):
        return int(self.lib.sc_tucker_chain_t3m_bytes(byref(TuckerChainDesc(*dims))))

    def tucker_chain_forward_fused(self, dims, xhat, u_in, t3, u_out, t3m, z, t, yhat, stream=0):
        """t3m (n_modes, r_in, r_out): written here, read by tucker_chain_backward_fused"""
        self._check(self.lib.sc_tucker_chain_forward_fused(byref(TuckerChainDesc(*dims)), xhat, u_in, t3, u_out, t3m, z, t,
                                                           yhat, stream))

    def tucker_chain_backward_fused_workspace_bytes(self, dims):
        return int(self.lib.sc_tucker_chain_backward_fused_workspace_bytes(byref(TuckerChainDesc(*dims))))

    def tucker_chain_backward_fused(self, dims, xhat, u_in, t3m, u_out, z, t, gy, gxhat, gu_in, gt3, gu_out, ws, ws_bytes,
                                    stream=0):
        """gt3 is required; null (0) gxhat / gu_in / gu_out skip that gradient"""
        self._check(self.lib.sc_tucker_chain_backward_fused(byref(TuckerChainDesc(*dims)), xhat, u_in, t3m, u_out, z, t, gy,
                                                            gxhat, gu_in, gt3, gu_out, ws, ws_bytes, stream))

    def round_f16(self, in_ptr, out_ptr, n, stream=0):
        """out = float16(in) in fp32 storage (the cast points of fno_block_precision half / mixed)."""
        self._check(self.lib.sc_round_f16(in_ptr, out_ptr, n, stream))

    def wire_pack_c32(self, spec_ptr, wire_ptr, n, c, k1, rest, P, rows, w0, stream=0):
        """complex64 [n, c, k1, rest] -> complex32 wire [P, n, c, rows, rest]: spectrum row r on global wire row w0 + r,
        every other wire row zero"""
        self._check(self.lib.sc_wire_pack_c32(spec_ptr, wire_ptr, n, c, k1, rest, P, rows, w0, stream))

    def wire_unpack_c32(self, wire_ptr, spec_ptr, n, c, k1, rest, P, rows, w0, stream=0):
        """complex32 wire [P, n, c, rows, rest] -> complex64 [n, c, k1, rest]: rows [w0, w0 + k1) of the P * rows
        concatenation"""
        self._check(self.lib.sc_wire_unpack_c32(wire_ptr, spec_ptr, n, c, k1, rest, P, rows, w0, stream))

    def bicubic_rows_forward(self, x_ptr, y_ptr, images, rows_in, w_in, src_row0, h_in, h_out, w_out, out_row0,
                             rows_out, stream=0):
        """rows [out_row0, + rows_out) of the bicubic (align_corners) resample of a global (h_in, w_in) grid to
        (h_out, w_out), from its rows [src_row0, + rows_in)"""
        self._check(self.lib.sc_bicubic_rows_forward(x_ptr, y_ptr, images, rows_in, w_in, src_row0, h_in, h_out, w_out,
                                                     out_row0, rows_out, stream))

    def bicubic_rows_backward(self, gy_ptr, gx_ptr, images, rows_in, w_in, src_row0, h_in, h_out, w_out, out_row0,
                              rows_out, stream=0):
        """gx (images, rows_in, w_in) overwritten with the adjoint of bicubic_rows_forward applied to gy"""
        self._check(self.lib.sc_bicubic_rows_backward(gy_ptr, gx_ptr, images, rows_in, w_in, src_row0, h_in, h_out,
                                                      w_out, out_row0, rows_out, stream))

    def legendre_analysis(self, x_ptr, tab_ptr, c_ptr, lines, nlat, lmax, mmax, stream=0):
        """c (lines, lmax, mmax) = sum over k of x (lines, nlat, mmax) times the real table (lmax, nlat, mmax)"""
        self._check(self.lib.sc_legendre_analysis(x_ptr, tab_ptr, c_ptr, lines, nlat, lmax, mmax, stream))

    def legendre_synthesis(self, c_ptr, tab_ptr, x_ptr, lines, nlat, lmax, mmax, stream=0):
        """x (lines, nlat, mmax) = sum over l of c (lines, lmax, mmax) times the real table (lmax, nlat, mmax)"""
        self._check(self.lib.sc_legendre_synthesis(c_ptr, tab_ptr, x_ptr, lines, nlat, lmax, mmax, stream))

    def spectral_op(self, x_ptr, y_ptr, *, kept, groups, n_src, n_out, terms, tabs_a, tabs_b, n_tab, y_group_stride,
                    y_out_stride, conj=False, stream=0):
        """yhat[g, t] = sum over terms (src, out, coef, tab rows per axis) with out = t of
        coef * (prod_d A_d[tab_d] + prod_d B_d[tab_d]) / 2 * xhat[g, src] (sc_spectral_op); tabs_a / tabs_b the device
        pointers of the per-axis tables [n_tab_d][kept_d] complex64"""
        d = SpecopDesc()
        nd = len(kept)
        if len(terms) > SC_SPECOP_MAX_TERMS or not 1 <= nd <= 3:
            raise EngineError(f"sc_spectral_op: {len(terms)} terms over {nd} dims (at most {SC_SPECOP_MAX_TERMS} terms "
                              "of 1 to 3 dims per call)")
        d.ndim, d.n_src, d.n_out, d.n_terms, d.conj = nd, n_src, n_out, len(terms), int(bool(conj))
        d.groups, d.y_group_stride, d.y_out_stride = groups, y_group_stride, y_out_stride
        for i in range(nd):
            d.kept[i], d.n_tab[i], d.A[i], d.B[i] = kept[i], n_tab[i], tabs_a[i], tabs_b[i]
        for j, (src, out, coef, tab) in enumerate(terms):
            d.term_src[j], d.term_out[j], d.term_coef[j] = src, out, coef
            for i in range(nd):
                d.term_tab[j][i] = tab[i]
        self._check(self.lib.sc_spectral_op(byref(d), x_ptr, y_ptr, stream))

    def helmholtz_project(self, x_ptr, y_ptr, *, kept, groups, sel, eps, tabs, y_group_stride, y_comp_stride, stream=0):
        """yhat[g, a] = sum_b 1/2 (G+_ab + G-_ab) xhat[g, b] with the per-mode projector G of sc_helmholtz_project;
        tabs the device pointers of the per-axis tables [kept_d][2][3] fp32, sel the axis whose wavenumber each
        component takes; y_ptr may equal x_ptr"""
        d = HelmholtzDesc()
        nd = len(kept)
        if not 2 <= nd <= 3 or len(sel) != nd or len(tabs) != nd:
            raise EngineError(f"sc_helmholtz_project: {nd} dims with {len(sel)} sel entries and {len(tabs)} tables "
                              "(2 or 3 dims, one of each per dim)")
        d.ndim, d.eps, d.groups = nd, eps, groups
        d.y_group_stride, d.y_comp_stride = y_group_stride, y_comp_stride
        for i in range(nd):
            d.kept[i], d.sel[i], d.T[i] = kept[i], sel[i], tabs[i]
        self._check(self.lib.sc_helmholtz_project(byref(d), x_ptr, y_ptr, stream))

    def band_apply(self, u_ptr, u2_ptr, y_ptr, *, dims, periodic, groups, n_src, n_out, terms, tabs, n_tab,
                   y_group_stride, y_out_stride, scale=0, scale_mul=0, stream=0):
        """y[g, t] = scale[g] scale_mul sum over terms (src, out, coef, axis, tab) with out = t of coef * (banded
        matrix tab of the axis, or the identity for axis -1) applied to u[g, src] (- u2[g, src]) (sc_band_apply); tabs
        the device pointers of the per-axis tables [n_tab_d][dims_d][7] fp32"""
        d = BandDesc()
        nd = len(dims)
        if len(terms) > SC_BAND_MAX_TERMS or not 1 <= nd <= 3:
            raise EngineError(f"sc_band_apply: {len(terms)} terms over {nd} dims (at most {SC_BAND_MAX_TERMS} terms of "
                              "1 to 3 dims per call)")
        d.ndim, d.n_src, d.n_out, d.n_terms = nd, n_src, n_out, len(terms)
        d.groups, d.y_group_stride, d.y_out_stride = groups, y_group_stride, y_out_stride
        d.scale, d.scale_mul = scale or None, scale_mul or None
        for i in range(nd):
            d.dims[i], d.periodic[i], d.n_tab[i], d.T[i] = dims[i], int(bool(periodic[i])), n_tab[i], tabs[i] or None
        for j, (src, out, coef, axis, tab) in enumerate(terms):
            d.term_src[j], d.term_out[j], d.term_coef[j], d.term_axis[j], d.term_tab[j] = src, out, coef, axis, tab
        self._check(self.lib.sc_band_apply(byref(d), u_ptr or None, u2_ptr or None, y_ptr or None, stream))

    @staticmethod
    def sobolev_desc(*, dims, periodic=None, lines, h1, p=2, relative=True, take_root=True, reduce_mean=False,
                     konst=1.0, eps=0.0, tabs=None, chunks=0):
        d = SobolevDesc()
        d.ndim, d.h1, d.p, d.relative, d.take_root = len(dims), int(bool(h1)), int(p), int(bool(relative)), int(bool(take_root))
        d.reduce_mean, d.chunks, d.lines, d.konst, d.eps = int(bool(reduce_mean)), int(chunks), int(lines), konst, eps
        if not 1 <= len(dims) <= 3:
            raise EngineError(f"sc_sobolev_sums: {len(dims)} dims (1 to 3)")
        for i in range(len(dims)):
            d.dims[i] = dims[i]
            d.periodic[i] = 1 if periodic is None else int(bool(periodic[i]))
            d.T[i] = (tabs[i] or None) if tabs is not None else None
        return d

    def sobolev_workspace_bytes(self, desc):
        return int(self.lib.sc_sobolev_workspace_bytes(byref(desc)))

    def sobolev_sums(self, desc, x_ptr, y_ptr, ws_ptr, ws_bytes, v_ptr, dv_ptr, loss_ptr, stream=0):
        """the per-line norms v, their derivatives dv by the numerator sums (times the reduction factor) and the
        reduced loss of LpLoss / H1Loss: two launches (sc_sobolev_sums)"""
        self._check(self.lib.sc_sobolev_sums(byref(desc), x_ptr or None, y_ptr or None, ws_ptr or None, ws_bytes,
                                             v_ptr or None, dv_ptr or None, loss_ptr or None, stream))

    def lp_grad(self, desc, x_ptr, y_ptr, dv_ptr, gout_ptr, gx_ptr, stream=0):
        """gx[l, i] = dv[l] gout p |x - y|^(p-1) sign(x - y) (sc_lp_grad)"""
        self._check(self.lib.sc_lp_grad(byref(desc), x_ptr or None, y_ptr or None, dv_ptr or None, gout_ptr or None,
                                        gx_ptr or None, stream))

    @staticmethod
    def radius_desc(d, n, m, radius, return_norm=False):
        r = RadiusDesc()
        r.d, r.return_norm, r.n, r.m, r.radius = int(d), int(bool(return_norm)), int(n), int(m), float(radius)
        return r

    def radius_count(self, desc, data_ptr, queries_ptr, deg_ptr, splits_ptr, stream=0):
        """deg[m] and the exclusive scan row_splits[m + 1] of a fixed-radius search (sc_radius_count)"""
        self._check(self.lib.sc_radius_count(byref(desc), data_ptr or None, queries_ptr or None, deg_ptr or None,
                                             splits_ptr or None, stream))

    def radius_fill(self, desc, data_ptr, queries_ptr, splits_ptr, n_edges, index_ptr, weights_ptr, stream=0):
        """neighbors_index[n_edges] (ascending per query) and the squared distances (sc_radius_fill)"""
        self._check(self.lib.sc_radius_fill(byref(desc), data_ptr or None, queries_ptr or None, splits_ptr or None,
                                            n_edges, index_ptr or None, weights_ptr or None, stream))

    def radius_grid_workspace_bytes(self, desc):
        return int(self.lib.sc_radius_grid_workspace_bytes(byref(desc)))

    def radius_grid_count(self, desc, data_ptr, queries_ptr, deg_ptr, splits_ptr, ws_ptr, ws_bytes, stream=0):
        """radius_count over a uniform cell grid built in ws (sc_radius_grid_count)"""
        self._check(self.lib.sc_radius_grid_count(byref(desc), data_ptr or None, queries_ptr or None, deg_ptr or None,
                                                  splits_ptr or None, ws_ptr or None, ws_bytes, stream))

    def radius_grid_fill(self, desc, data_ptr, queries_ptr, splits_ptr, n_edges, index_ptr, weights_ptr, ws_ptr, ws_bytes,
                         stream=0):
        """radius_fill over the grid the count pass left in ws (sc_radius_grid_fill)"""
        self._check(self.lib.sc_radius_grid_fill(byref(desc), data_ptr or None, queries_ptr or None, splits_ptr or None,
                                                 n_edges, index_ptr or None, weights_ptr or None, ws_ptr or None,
                                                 ws_bytes, stream))

    @staticmethod
    def csr_desc(rows, cols, n_edges, n_splits=None):
        d = CsrDesc()
        d.rows, d.cols, d.n_edges = int(rows), int(cols), int(n_edges)
        d.n_splits = int(rows) + 1 if n_splits is None else int(n_splits)
        return d

    def csr_transpose_workspace_bytes(self, desc):
        return int(self.lib.sc_csr_transpose_workspace_bytes(byref(desc)))

    def csr_transpose(self, desc, splits_ptr, index_ptr, col_splits_ptr, perm_ptr, row_ptr, ws_ptr, ws_bytes, stream=0):
        self._check(self.lib.sc_csr_transpose(byref(desc), splits_ptr or None, index_ptr or None, col_splits_ptr or None,
                                              perm_ptr or None, row_ptr or None, ws_ptr or None, ws_bytes, stream))

    @staticmethod
    def csr_reduce_desc(*, rows, n_edges, channels, splits, n_splits=None, batch=1, mean=False, n_f=0, n_scale_rows=0,
                        k_batch_stride=0, f_batch_stride=0, perm=0, gather64=0, gather32=0, scale_splits=0, w=0):
        d = CsrReduceDesc()
        d.rows, d.n_edges, d.channels, d.batch, d.mean = int(rows), int(n_edges), int(channels), int(batch), int(bool(mean))
        d.n_splits = int(rows) + 1 if n_splits is None else int(n_splits)
        d.n_f, d.n_scale_rows, d.k_batch_stride, d.f_batch_stride = int(n_f), int(n_scale_rows), int(k_batch_stride), int(f_batch_stride)
        d.splits, d.perm, d.gather64, d.gather32 = splits or None, perm or None, gather64 or None, gather32 or None
        d.scale_splits, d.w = scale_splits or None, w or None
        return d

    def csr_reduce(self, desc, k_ptr, f_ptr, out_ptr, stream=0):
        """out[b, i] = s_i sum over the segment of K F w (sc_csr_reduce)"""
        self._check(self.lib.sc_csr_reduce(byref(desc), k_ptr or None, f_ptr or None, out_ptr or None, stream))

    def csr_edge_grad(self, desc, g_ptr, f_ptr, gk_ptr, stream=0):
        """gK[(b,) e] = s_i w[e] g[b, i] F[b, row(e)] (sc_csr_edge_grad)"""
        self._check(self.lib.sc_csr_edge_grad(byref(desc), g_ptr or None, f_ptr or None, gk_ptr or None, stream))

    @staticmethod
    def edge_lift_desc(*, rows, n_edges, n_py, channels, splits, index, batch=1, py_batch_stride=0, act=SC_LIFT_IDENTITY,
                       n_splits=None):
        d = EdgeLiftDesc()
        d.rows, d.n_edges, d.n_py, d.channels, d.batch, d.act = int(rows), int(n_edges), int(n_py), int(channels), int(batch), int(act)
        d.n_splits = int(rows) + 1 if n_splits is None else int(n_splits)
        d.py_batch_stride, d.splits, d.index = int(py_batch_stride), splits or None, index or None
        return d

    def edge_lift(self, desc, py_ptr, px_ptr, bias_ptr, h_ptr, stream=0):
        """H[(b,) e] = act(Py[(b,) index[e]] + Px[row(e)] + bias) (sc_edge_lift)"""
        self._check(self.lib.sc_edge_lift(byref(desc), py_ptr or None, px_ptr or None, bias_ptr or None, h_ptr or None,
                                          stream))

    def edge_lift_bwd(self, desc, py_ptr, px_ptr, bias_ptr, gh_ptr, gpre_ptr, stream=0):
        """gPre = gH act'(pre), the pre-activation recomputed (sc_edge_lift_bwd)"""
        self._check(self.lib.sc_edge_lift_bwd(byref(desc), py_ptr or None, px_ptr or None, bias_ptr or None,
                                              gh_ptr or None, gpre_ptr or None, stream))

    @staticmethod
    def edge_mlp_desc(*, rows, n_edges, n_py, widths, splits, index, batch=1, py_batch_stride=0, chunk_edges=0,
                      row_of_edge=0, col_splits=0, perm=0, n_layers=None, n_splits=None):
        """widths: the output channels of the n_layers Linear layers, the point-wise layer 0 first"""
        d = EdgeMlpDesc()
        d.rows, d.n_edges, d.n_py, d.batch = int(rows), int(n_edges), int(n_py), int(batch)
        d.n_splits = int(rows) + 1 if n_splits is None else int(n_splits)
        d.py_batch_stride, d.chunk_edges = int(py_batch_stride), int(chunk_edges)
        d.n_layers = len(widths) if n_layers is None else int(n_layers)
        for i, w in enumerate(list(widths)[:SC_EDGE_MLP_MAX_LAYERS]):
            d.widths[i] = int(w)
        d.splits, d.index, d.row_of_edge = splits or None, index or None, row_of_edge or None
        d.col_splits, d.perm = col_splits or None, perm or None
        return d

    def edge_mlp_workspace_bytes(self, desc):
        return int(self.lib.sc_edge_mlp_workspace_bytes(byref(desc)))

    @staticmethod
    def _ptr_array(ptrs):
        return (c_void_p * max(len(ptrs), 1))(*[p or None for p in ptrs])

    def edge_mlp_forward(self, desc, py_ptr, px_ptr, bias0_ptr, w_ptrs, b_ptrs, k_ptr, ws_ptr, ws_bytes, stream=0):
        """K = the kernel MLP over chunks of edges (sc_edge_mlp_forward); w_ptrs / b_ptrs: device pointers of layers 1 .."""
        self._check(self.lib.sc_edge_mlp_forward(byref(desc), py_ptr or None, px_ptr or None, bias0_ptr or None,
                                                 self._ptr_array(w_ptrs), self._ptr_array(b_ptrs), k_ptr or None,
                                                 ws_ptr or None, ws_bytes, stream))

    def edge_mlp_backward(self, desc, py_ptr, px_ptr, bias0_ptr, w_ptrs, b_ptrs, gk_ptr, gpy_ptr, gpx_ptr, gw_ptrs,
                          gb_ptrs, ws_ptr, ws_bytes, stream=0):
        """gPy, gPx, gW_l, gb_l of the kernel MLP, the chain recomputed per chunk (sc_edge_mlp_backward)"""
        self._check(self.lib.sc_edge_mlp_backward(byref(desc), py_ptr or None, px_ptr or None, bias0_ptr or None,
                                                  self._ptr_array(w_ptrs), self._ptr_array(b_ptrs), gk_ptr or None,
                                                  gpy_ptr or None, gpx_ptr or None, self._ptr_array(gw_ptrs),
                                                  self._ptr_array(gb_ptrs), ws_ptr or None, ws_bytes, stream))

    @staticmethod
    def fdconv_desc(*, dims, batch, c_in, c_out, k, groups=1, padding="periodic", inv_h=1.0):
        d = FdconvDesc()
        d.ndim, d.k, d.groups = len(dims), int(k), int(groups)
        d.padding = SC_FDCONV_PADDING[padding] if isinstance(padding, str) else int(padding)
        for i, n in enumerate(dims[:3]):
            d.dims[i] = int(n)
        d.batch, d.c_in, d.c_out, d.inv_h = int(batch), int(c_in), int(c_out), float(inv_h)
        return d

    def fdconv_path(self, desc):
        """the route of a descriptor: SC_FDCONV_PATH_GENERAL, SC_FDCONV_PATH_MFMA, or 0 where it is refused"""
        return int(self.lib.sc_fdconv_path(byref(desc)))

    def fdconv_workspace_bytes(self, desc):
        return int(self.lib.sc_fdconv_workspace_bytes(byref(desc)))

    def fdconv_forward_workspace_bytes(self, desc):
        """what sc_fdconv_forward needs: the folded weights alone"""
        return int(self.lib.sc_fdconv_forward_workspace_bytes(byref(desc)))

    def fdconv_forward(self, desc, x_ptr, w_ptr, y_ptr, ws_ptr, ws_bytes, stream=0):
        """y = (conv_pad(x, W) - conv_1x1(x, sum_taps W)) inv_h as one folded convolution (sc_fdconv_forward)"""
        self._check(self.lib.sc_fdconv_forward(byref(desc), x_ptr or None, w_ptr or None, y_ptr or None, ws_ptr or None,
                                               ws_bytes, stream))

    def fdconv_backward(self, desc, x_ptr, w_ptr, gout_ptr, gx_ptr, gw_ptr, ws_ptr, ws_bytes, stream=0):
        """gx and / or gw of sc_fdconv_forward (a zero pointer: not wanted)"""
        self._check(self.lib.sc_fdconv_backward(byref(desc), x_ptr or None, w_ptr or None, gout_ptr or None,
                                                gx_ptr or None, gw_ptr or None, ws_ptr or None, ws_bytes, stream))

    @staticmethod
    def disco_desc(*, batch, c_in, c_out, in_shape, out_shape, basis, support, stride=(1, 1), padding=(0, 0),
                   output_padding=(0, 0), groups=1, q_weight=1.0, transposed=False):
        d = DiscoDesc()
        d.batch, d.c_in, d.c_out, d.groups, d.basis = int(batch), int(c_in), int(c_out), int(groups), int(basis)
        (d.h_in, d.w_in), (d.h_out, d.w_out) = map(int, in_shape), map(int, out_shape)
        (d.ph, d.pw), (d.sh, d.sw) = map(int, support), map(int, stride)
        (d.pad_h, d.pad_w), (d.opad_h, d.opad_w) = map(int, padding), map(int, output_padding)
        d.transposed, d.q_weight = int(transposed), float(q_weight)
        return d

    def disco_path(self, desc):
        """the route of a descriptor: SC_DISCO_PATH_GENERAL, SC_DISCO_PATH_MFMA, or 0 where it is refused"""
        return int(self.lib.sc_disco_path(byref(desc)))

    def disco_workspace_bytes(self, desc):
        return int(self.lib.sc_disco_workspace_bytes(byref(desc)))

    def disco_forward_workspace_bytes(self, desc):
        """what sc_disco_forward needs: the folded kernels alone"""
        return int(self.lib.sc_disco_forward_workspace_bytes(byref(desc)))

    def disco_forward(self, desc, x_ptr, w_ptr, psi_ptr, bias_ptr, y_ptr, ws_ptr, ws_bytes, stream=0):
        """y = conv2d / conv_transpose2d(x, q sum_k psi[k] weight[.., k], bias) (sc_disco_forward)"""
        self._check(self.lib.sc_disco_forward(byref(desc), x_ptr or None, w_ptr or None, psi_ptr or None,
                                              bias_ptr or None, y_ptr or None, ws_ptr or None, ws_bytes, stream))

    def disco_backward(self, desc, x_ptr, w_ptr, psi_ptr, gout_ptr, gx_ptr, gw_ptr, gbias_ptr, ws_ptr, ws_bytes,
                       stream=0):
        """gx, gw and / or gbias of sc_disco_forward (a zero pointer: not wanted)"""
        self._check(self.lib.sc_disco_backward(byref(desc), x_ptr or None, w_ptr or None, psi_ptr or None,
                                               gout_ptr or None, gx_ptr or None, gw_ptr or None, gbias_ptr or None,
                                               ws_ptr or None, ws_bytes, stream))

    @staticmethod
    def dsparse_desc(*, batch, c_in, c_out, n_in, n_out, nnz, basis, groups=1):
        d = DsparseDesc()
        d.batch, d.c_in, d.c_out, d.n_in, d.n_out, d.nnz = int(batch), int(c_in), int(c_out), int(n_in), int(n_out), int(nnz)
        d.groups, d.basis = int(groups), int(basis)
        return d

    @staticmethod
    def dsparse_csr(splits_ptr, cols_ptr, vals_ptr, rows, nnz):
        """a CSR form of Psi for sc_dsparse_*: int32 splits (rows + 1) and columns, fp32 values, as raw pointers"""
        return DsparseCsr(splits_ptr or None, cols_ptr or None, vals_ptr or None, int(rows), int(nnz))

    def dsparse_path(self, desc):
        """the route of a descriptor: SC_DSPARSE_PATH_GENERAL, SC_DSPARSE_PATH_MFMA, or 0 where it is refused"""
        return int(self.lib.sc_dsparse_path(byref(desc)))

    def dsparse_workspace_bytes(self, desc):
        return int(self.lib.sc_dsparse_workspace_bytes(byref(desc)))

    def dsparse_forward_workspace_bytes(self, desc):
        return int(self.lib.sc_dsparse_forward_workspace_bytes(byref(desc)))

    def dsparse_forward(self, desc, csr, x_ptr, q_ptr, w_ptr, bias_ptr, out_ptr, z_ptr, ws_ptr, ws_bytes, stream=0):
        """out = contraction of Z = Psi (q x) with the weight, + bias; Z (n_out, batch, basis, c_in) is written too"""
        self._check(self.lib.sc_dsparse_forward(byref(desc), byref(csr), x_ptr or None, q_ptr or None, w_ptr or None,
                                                bias_ptr or None, out_ptr or None, z_ptr or None, ws_ptr or None,
                                                ws_bytes, stream))

    def dsparse_backward(self, desc, csr_t, q_ptr, w_ptr, z_ptr, gout_ptr, gx_ptr, gw_ptr, gbias_ptr, ws_ptr, ws_bytes,
                         stream=0):
        """gx, gw and / or gbias of sc_dsparse_forward (a zero pointer: not wanted)"""
        self._check(self.lib.sc_dsparse_backward(byref(desc), byref(csr_t) if csr_t is not None else None, q_ptr or None,
                                                 w_ptr or None, z_ptr or None, gout_ptr or None, gx_ptr or None,
                                                 gw_ptr or None, gbias_ptr or None, ws_ptr or None, ws_bytes, stream))

    @staticmethod
    def attn_desc(*, batch, n_src, n_qry, heads, head_dim, rotary=0, has_weights=0):
        d = AttnDesc()
        d.batch, d.n_src, d.n_qry = int(batch), int(n_src), int(n_qry)
        d.heads, d.head_dim, d.rotary, d.has_weights = int(heads), int(head_dim), int(rotary), int(has_weights)
        return d

    def attn_path(self, desc):
        """the route of a descriptor: SC_ATTN_PATH_VECTOR, SC_ATTN_PATH_MFMA, or 0 where it is refused"""
        return int(self.lib.sc_attn_path(byref(desc)))

    def attn_workspace_bytes(self, desc):
        return int(self.lib.sc_attn_workspace_bytes(byref(desc)))

    def attn_forward(self, desc, q_ptr, k_ptr, v_ptr, pos_src_ptr, pos_qry_ptr, inv_freq_ptr, rot_scale, w_ptr, u_ptr,
                     dots_ptr, ws_ptr, ws_bytes, stream=0):
        """u = ((R q) dots) w with dots = sum_n (R LN(k))^T LN(v); u and dots are written"""
        self._check(self.lib.sc_attn_forward(byref(desc), q_ptr or None, k_ptr or None, v_ptr or None,
                                             pos_src_ptr or None, pos_qry_ptr or None, inv_freq_ptr or None,
                                             float(rot_scale), w_ptr or None, u_ptr or None, dots_ptr or None,
                                             ws_ptr or None, ws_bytes, stream))

    def attn_backward(self, desc, q_ptr, k_ptr, v_ptr, pos_src_ptr, pos_qry_ptr, inv_freq_ptr, rot_scale, w_ptr,
                      dots_ptr, gu_ptr, gq_ptr, gk_ptr, gv_ptr, ws_ptr, ws_bytes, stream=0):
        """gq, gk and / or gv of sc_attn_forward (a zero pointer: not wanted)"""
        self._check(self.lib.sc_attn_backward(byref(desc), q_ptr or None, k_ptr or None, v_ptr or None,
                                              pos_src_ptr or None, pos_qry_ptr or None, inv_freq_ptr or None,
                                              float(rot_scale), w_ptr or None, dots_ptr or None, gu_ptr or None,
                                              gq_ptr or None, gk_ptr or None, gv_ptr or None, ws_ptr or None, ws_bytes,
                                              stream))

    @staticmethod
    def knn_desc(d, n, m, k):
        r = KnnDesc()
        r.d, r.k, r.n, r.m = int(d), int(k), int(n), int(m)
        return r

    def knn(self, desc, data_ptr, queries_ptr, index_ptr, d2_ptr, stream=0):
        """index[m, k] and d2[m, k] of every query's k nearest data points, ascending (d2, data index) (sc_knn)"""
        self._check(self.lib.sc_knn(byref(desc), data_ptr or None, queries_ptr or None, index_ptr or None,
                                    d2_ptr or None, stream))

    @staticmethod
    def nufd_desc(*, n, k, n_deriv=1, batch=1, d=1, deriv=(), radius=None, lam=0.0):
        r = NufdDesc()
        r.n, r.d, r.k, r.n_deriv, r.batch = int(n), int(d), int(k), int(n_deriv), int(batch)
        for i, v in enumerate(list(deriv)[:8]):
            r.deriv[i] = int(v)
        r.has_radius, r.radius, r.lam = int(radius is not None), float(radius or 0.0), float(lam)
        return r

    def nufd_weights(self, desc, points_ptr, index_ptr, d2_ptr, weights_ptr, flag_ptr, stream=0):
        """weights[n, n_deriv, k] of the point-cloud finite differences and flag[n] of the ill-posed points"""
        self._check(self.lib.sc_nufd_weights(byref(desc), points_ptr or None, index_ptr or None, d2_ptr or None,
                                             weights_ptr or None, flag_ptr or None, stream))

    def nufd_apply(self, desc, weights_ptr, index_ptr, values_ptr, out_ptr, stream=0):
        """out[j, b, p] = sum_m weights[p, j, m] values[b, index[p, m]]"""
        self._check(self.lib.sc_nufd_apply(byref(desc), weights_ptr or None, index_ptr or None, values_ptr or None,
                                           out_ptr or None, stream))

    def nufd_apply_adjoint(self, desc, weights_ptr, col_splits_ptr, perm_ptr, gout_ptr, gvalues_ptr, stream=0):
        """gvalues[b, q] = sum over the stencil entries that name q (sc_csr_transpose order) of w gout"""
        self._check(self.lib.sc_nufd_apply_adjoint(byref(desc), weights_ptr or None, col_splits_ptr or None,
                                                   perm_ptr or None, gout_ptr or None, gvalues_ptr or None, stream))

    def modegemm_msum(self, a_ptr, b_ptr, c_ptr, stream=0, **kw):
        self._check(self.lib.sc_modegemm_msum(byref(self._gemm_desc(kw)), a_ptr, b_ptr, c_ptr, stream))

    def modegemm_msum_workspace_bytes(self, **kw):
        """Bytes of workspace sc_modegemm_msum_ws needs for this problem (0: empty problem)."""
        return int(self.lib.sc_modegemm_msum_workspace_bytes(byref(self._gemm_desc(kw))))

    def modegemm_msum_path(self, **kw):
        """1: sc_modegemm_msum_ws runs the matrix-core kernel, 0: the slot form of the VALU kernel."""
        return int(self.lib.sc_modegemm_msum_path(byref(self._gemm_desc(kw))))

    def modegemm_msum_ws(self, a_ptr, b_ptr, c_ptr, ws_ptr, ws_bytes, stream=0, **kw):
        """C[p, q] = sum over modes and r, OVERWRITTEN (matrix-core kernel + fixed-order reduction)."""
        self._check(self.lib.sc_modegemm_msum_ws(byref(self._gemm_desc(kw)), a_ptr, b_ptr, c_ptr, ws_ptr, ws_bytes, stream))

    def modegemm_uses_matrix_cores(self, **kw):
        d = ModeGemmDesc()
        for k, v in kw.items():
            setattr(d, k, v)
        return bool(self.lib.sc_modegemm_uses_matrix_cores(byref(d)))

    def modegemm_path(self, **kw):
        """0 VALU kernel, 1 k_modegemm_mfma, 2 k_modegemm_s8 (for 16-byte aligned operands)."""
        d = ModeGemmDesc()
        for k, v in kw.items():
            setattr(d, k, v)
        return int(self.lib.sc_modegemm_path(byref(d)))

    def modegemm_policy(self, **kw):
        """Cache policy of the streamed route: -1 = another route; else bits 0-1 the store policy of C (0 plain, 1
        non-temporal, 2 write-through), bit 2 = A requested non-temporally, bit 3 = B (SC_GEMM_C_WT / _NT_A / _NT_B)."""
        d = ModeGemmDesc()
        for k, v in kw.items():
            setattr(d, k, v)
        return int(self.lib.sc_modegemm_policy(byref(d)))

    def adamw_step(self, p_ptr, g_ptr, m_ptr, v_ptr, n, is_complex, stream=0, *, lr, beta1, beta2, eps,
                   weight_decay, correct_bias, step):
        d = AdamwDesc(lr, beta1, beta2, eps, weight_decay, int(step), int(bool(correct_bias)), 0)
        self._check(self.lib.sc_adamw_step(byref(d), p_ptr, g_ptr, m_ptr, v_ptr, n, int(bool(is_complex)), stream))

    def bias_grad(self, plan, ghat_ptr, batch, channels, gbias_ptr, stream=0):
        self._check(self.lib.sc_bias_grad(plan, ghat_ptr, batch, channels, gbias_ptr, stream))

    # -- fused dense layer -------------------------------------------------------------
    @staticmethod
    def layer_desc(batch, cin, cout, w_extent, w_start):
        L = LayerDesc()
        L.batch, L.cin, L.cout = batch, cin, cout
        for i, (e, s) in enumerate(zip(w_extent, w_start)):
            L.w_extent[i] = int(e)
            L.w_start[i] = int(s)
        return L

    def layer_workspace_bytes(self, plan, L):
        return int(self.lib.sc_layer_workspace_bytes(plan, byref(L)))

    def layer_forward(self, plan, L, x, w, bias, y, xhat_saved, ws, stream=0):
        self._check(self.lib.sc_layer_forward(plan, byref(L), x, w, bias, y, xhat_saved, ws,
                                              stream))

    def layer_forward_ex(self, plan, L, x, w, bias, skip, preact, act, y, xhat_saved, ws, stream=0):
        """forward with the block epilogue y = act(layer(x) + skip) (include/sc_engine.h, sc_epilogue)"""
        ep = Epilogue(skip, preact, act, 0)
        self._check(self.lib.sc_layer_forward_ex(plan, byref(L), x, w, bias, byref(ep), y, xhat_saved, ws, stream))

    def transform_inverse_ex(self, plan, mode, yhat_ptr, bias_ptr, channels, skip, preact, act, y_ptr, n_images,
                             ws_ptr, stream=0):
        ep = Epilogue(skip, preact, act, 0)
        self._check(self.lib.sc_transform_inverse_ex(plan, mode, yhat_ptr, bias_ptr, channels, byref(ep), y_ptr,
                                                     n_images, ws_ptr, stream))

    def layer_backward(self, plan, L, gy, xhat_saved, w, gx, gw, gbias, ws, stream=0):
        self._check(self.lib.sc_layer_backward(plan, byref(L), gy, xhat_saved, w, gx, gw,
                                               gbias, ws, stream))

    def layer_backward_ex(self, plan, L, gy, xhat_saved, w, gx, gw, gbias, gx_addend, ws, stream=0):
        self._check(self.lib.sc_layer_backward_ex(plan, byref(L), gy, xhat_saved, w, gx, gw, gbias, gx_addend, ws, stream))


_LIB = None


def get_lib():
    """The product's engine library (HIP build); raises EngineError when it is not built."""
    global _LIB
    if _LIB is None:
        # SC_ENGINE_LIB: another BUILD of the same engine (scripts/build_variants.py: A-B measurements of compile-time
        # switches through the whole module stack); a missing file fails as loudly as a missing default library
        _LIB = ScEngineLib(os.environ.get("SC_ENGINE_LIB") or DEFAULT_LIB)
    return _LIB
