"""Host-side Python mirror of the GPU-NTT operator interface on top of libgpuntt.so.

The product is the C++/HIP library (gpu-ntt_amd/csrc -> gpu-ntt_amd/lib/libgpuntt.so, C ABI
in include/gpuntt_c.h).  This module only binds that C ABI with ctypes so tests, bench.py and
multi-GPU drivers can call the same entry points with the reference's names and argument
meaning (reference src/include/gpuntt/ntt_merge/ntt.cuh:315-421,
src/include/gpuntt/ntt_4step/ntt_4step.cuh:46-49,278-308):

    GPU_NTT / GPU_INTT / GPU_NTT_Inplace / GPU_INTT_Inplace   (single modulus or RNS)
    GPU_4STEP_NTT / GPU_Transpose
    GPU_Automorphism_NTT / GPU_Automorphism (extension: Galois automorphisms, gpuntt/ntt_merge/galois.cuh)
    BaseConvPlan / baseconv_constants (extension: RNS fast base conversion, gpuntt/rns/base_conversion.cuh)
    InnerProductPlan / innerprod_constants / innerprod_reference (extension: RNS inner product,
    gpuntt/rns/inner_product.cuh)
    KeySwitchPlan / keyswitch_constants / keyswitch_scratch_bytes / keyswitch_hoisted_scratch_bytes /
    keyswitch_hoisted_sum_scratch_bytes / keyswitch_reference_mod_up / keyswitch_reference_mod_down (extension: hybrid
    key switching, gpuntt/rns/key_switch.cuh)
    Modulus, ntt_configuration, ntt_rns_configuration, ntt4step_configuration,
    ntt4step_rns_configuration, NTTParameters, NTTParameters4Step

Device buffers are torch tensors (torch is used for device memory and streams only);
64-bit words are carried in int64 tensors, 32-bit words in int32 tensors -- the library
reinterprets the bits as unsigned unless a signed dtype is requested explicitly.

There is NO CPU fallback: importing works anywhere, but every compute entry point raises
if libgpuntt.so is missing or no GPU is present.
"""
import ctypes
import os
import subprocess
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPUNTT_LIB: an alternative build of the library (A/B experiments under tools/: same sources, one macro changed)
LIB_PATH = os.environ.get("GPUNTT_LIB") or os.path.join(_HERE, "lib", "libgpuntt.so")
CSRC = os.path.join(_HERE, "csrc")

# enum values (reference src/include/gpuntt/common/nttparameters.cuh:19-36)
FORWARD, INVERSE = 0, 1
PerPolynomial, PerCoefficient = 0, 1
X_N_plus, X_N_minus = 0, 1

GPUNTT_OK = 0
_ERR_INVALID, _ERR_HIP = -1, -2


class GpuNttError(RuntimeError):
    """HipException / CudaException of the C++ API (failed launch)."""


class _M32(ctypes.Structure):
    _fields_ = [("value", ctypes.c_uint32), ("bit", ctypes.c_uint32), ("mu", ctypes.c_uint32)]


class _M64(ctypes.Structure):
    _fields_ = [("value", ctypes.c_uint64), ("bit", ctypes.c_uint64), ("mu", ctypes.c_uint64)]


_lib = None


def build_library(jobs=8):
    """Compile every HIP source for gfx950 into gpu-ntt_amd/lib (hipcc cross-compiles
    without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j%d" % jobs])


def load_library():
    """dlopen libgpuntt.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            "%s not found: build it with `make -C gpu-ntt_amd/csrc -j8` "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    try:  # make sure the HIP runtime torch already loaded is the one we bind to
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the host-only helpers
        pass
    lib = ctypes.CDLL(LIB_PATH)
    lib.gpuntt_last_error.restype = ctypes.c_char_p
    for name in EXPORTED_SYMBOLS:
        getattr(lib, name)  # AttributeError if the ABI is incomplete
    _lib = lib
    for var, (opt, conv) in ENV_OPTIONS.items():
        if var in os.environ and "gpuntt_set_option" in EXPORTED_SYMBOLS:
            val = os.environ[var]
            set_option(opt, conv(val) if conv else val)
    return lib


# every symbol include/gpuntt_c.h declares
EXPORTED_SYMBOLS = ["gpuntt_last_error", "gpuntt_version"] + [
    "gpuntt_%s_%s" % (f, s)
    for f in ("modulus", "ntt", "intt", "ntt_rns", "intt_rns", "ntt_modulus_ordered",
              "ntt_poly_ordered", "polymul", "polymul_rns", "4step", "4step_rns", "4step_natural", "transpose",
              "merge_params",
              "4step_params", "plan_workspace_bytes", "plan_create", "plan_execute", "plan_fast_path",
              "plan_destroy", "operator_gpu", "4step_plan_workspace_bytes", "4step_plan_create",
              "4step_plan_execute", "4step_plan_fast_path", "4step_plan_destroy",
              "generate_power_table", "generate_4step_w", "butterfly_unit", "debug_recip_norm",
              "automorphism_ntt", "automorphism", "automorphism_rns",
              "baseconv_plan_workspace_bytes", "baseconv_plan_create", "baseconv_plan_convert",
              "baseconv_plan_convert_and_divide", "baseconv_plan_owns_workspace", "baseconv_plan_destroy",
              "baseconv_constants",
              "innerprod_plan_workspace_bytes", "innerprod_plan_create", "innerprod_plan_execute",
              "innerprod_plan_owns_workspace", "innerprod_plan_destroy", "innerprod_constants",
              "innerprod_reference",
              "keyswitch_plan_workspace_bytes", "keyswitch_plan_scratch_bytes", "keyswitch_plan_create",
              "keyswitch_plan_mod_up", "keyswitch_plan_mod_down", "keyswitch_plan_mod_down_add",
              "keyswitch_plan_relinearize", "keyswitch_plan_decompose",
              "keyswitch_plan_switch_digits", "keyswitch_plan_apply", "keyswitch_plan_hoisted_scratch_bytes",
              "keyswitch_plan_rotate_hoisted", "keyswitch_plan_hoisted_sum_scratch_bytes",
              "keyswitch_plan_rotate_hoisted_sum", "keyswitch_plan_multiply_relinearize",
              "keyswitch_plan_multiply_relinearize_sum", "keyswitch_plan_owns_workspace",
              "keyswitch_plan_destroy", "keyswitch_constants", "keyswitch_reference_mod_up",
              "keyswitch_reference_mod_down",
              "keyswitch_plan_workspace_bytes_rescale", "keyswitch_plan_create_rescale",
              "keyswitch_plan_rescale_limbs", "keyswitch_plan_rescale_scratch_bytes",
              "keyswitch_plan_mod_down_rescale", "keyswitch_plan_rescale",
              "keyswitch_plan_multiply_relinearize_rescale", "keyswitch_plan_multiply_relinearize_sum_rescale",
              "keyswitch_plan_rotate_hoisted_sum_rescale", "keyswitch_reference_mod_down_rescale",
              "keyswitch_reference_rescale",
              "keyswitch_plan_bsgs_scratch_bytes", "keyswitch_plan_linear_transform_bsgs",
              "keyswitch_plan_linear_transform_bsgs_rescale",
              "bfv_plan_workspace_bytes", "bfv_plan_scratch_bytes", "bfv_plan_create", "bfv_plan_extend",
              "bfv_plan_scale_round", "bfv_plan_multiply", "bfv_plan_multiply_relinearize", "bfv_plan_owns_workspace",
              "bfv_plan_destroy", "bfv_plan_max_terms", "bfv_plan_sum_scratch_bytes", "bfv_plan_multiply_sum",
              "bfv_plan_multiply_relinearize_sum", "bfv_max_terms",
              "bfv_constants", "bfv_reference_extend", "bfv_reference_scale_round",
              "sample_uniform", "sample_reference_uniform", "keyswitch_plan_lift_small",
              "keyswitch_plan_keygen_scratch_bytes", "keyswitch_plan_encrypt_scratch_bytes",
              "keyswitch_plan_generate_keys", "keyswitch_plan_encrypt_symmetric",
              "keyswitch_plan_phase_scratch_bytes", "keyswitch_plan_phase",
              "keyswitch_plan_encrypt_public_scratch_bytes", "keyswitch_plan_encrypt_public",
              "bfv_plan_scale_message", "bfv_plan_decode", "bfv_plan_decode_partials_bytes",
              "bfv_plan_decode_two_launch", "bfv_plan_decrypt_scratch_bytes", "bfv_plan_decrypt",
              "bfv_noise_budget_bits",
              "bfv_encoder_workspace_bytes", "bfv_encoder_scratch_bytes", "bfv_encoder_create", "bfv_encoder_encode",
              "bfv_encoder_decode", "bfv_encoder_owns_workspace", "bfv_encoder_destroy",
              "keyswitch_plan_lift_centred", "keyswitch_plan_multiply_plain")
    for s in ("u32", "u64")] + ["gpuntt_release_workspaces", "gpuntt_set_option", "gpuntt_galois_element_u32",
                                "gpuntt_automorphism_index_map", "gpuntt_philox4x32_10", "gpuntt_sample_small",
                                "gpuntt_sample_reference_small", "gpuntt_bfv_slot_maps"]

# GPUNTT_* environment variables of the A/B scripts and tests -> library options.  The C++ library reads no
# environment variable; this harness forwards them once, when it loads the library.
ENV_OPTIONS = {"GPUNTT_PATH": ("path", None), "GPUNTT_U32_E32": ("u32_e32", lambda v: int(v, 0)),
               "GPUNTT_TWO_SWEEP_BIG": ("two_sweep_big", None)}


TEST_HOOKS = {"no_scratch", "rns_force_fallback", "u32_e32", "reset_predictions", "two_sweep_big", "baseconv_ksplit",
              "keyswitch_split", "keyswitch_hoist_chunk", "contig_p4", "premul"}
TEST_PATHS = {"fast-strict", "generic-capped"}


def set_option(name, value):
    """GPU_NTT_SetOption (product options: path = default | generic | fast, check_4step_tables, rns_predict; names in
    include/gpuntt/ntt_merge/ntt.cuh).  The TEST HOOKS of this repository (csrc/test_hooks.h: path = fast-strict |
    generic-capped, no_scratch, rns_force_fallback, u32_e32) are not options of the public interface; this harness
    forwards them to gpuntt_test_set_hook so that the tests and tools/ keep one call."""
    name, value = str(name), str(value)
    if name in TEST_HOOKS or (name == "path" and value in TEST_PATHS):
        return set_test_hook(name, value)
    _check(load_library().gpuntt_set_option(name.encode(), value.encode()))


def set_test_hook(name, value):
    """gpuntt_test_set_hook (csrc/test_hooks.h)."""
    _check(load_library().gpuntt_test_set_hook(str(name).encode(), str(value).encode()))


def contig_p4_launches():
    """gpuntt_test_contig_p4_launches (csrc/test_hooks.h): launches of the four-polynomial tile of the forward 64-bit
    contiguous pass since the library was loaded."""
    fn = load_library().gpuntt_test_contig_p4_launches
    fn.restype = ctypes.c_ulonglong
    return int(fn())


def premul_launches():
    """gpuntt_test_premul_launches (csrc/test_hooks.h): calls since the library was loaded whose strided pass did the
    last pass's first twiddle product (forward 64-bit ring 2^16, hook premul)."""
    fn = load_library().gpuntt_test_premul_launches
    fn.restype = ctypes.c_ulonglong
    return int(fn())


def alloc_count():
    """gpuntt_test_alloc_count (csrc/test_hooks.h): hipMalloc / hipHostMalloc / hipFree / hipHostFree calls of the scratch
    chains and the family prediction's pool since the library was loaded."""
    fn = load_library().gpuntt_test_alloc_count
    fn.restype = ctypes.c_ulonglong
    return int(fn())


def scratch_stats():
    """gpuntt_test_scratch_stats (csrc/test_hooks.h): the twiddle scratch of captured calls, which their graph owns."""
    out = (ctypes.c_ulonglong * 6)()
    _check(load_library().gpuntt_test_scratch_stats(out))
    names = ("graph_owned", "died", "pooled", "reused", "chains_erased", "chains")
    return dict(zip(names, (int(v) for v in out)))


class launch_log:
    """with launch_log() as log: ...calls...; log.kernels -> the kernels the library enqueued inside the block, in order
    (gpuntt_test_launch_log_start / _take, csrc/test_hooks.h): ["prep_twiddles", "merge_pass_lazy:31", ...]"""

    def __enter__(self):
        _check(load_library().gpuntt_test_launch_log_start())
        self.kernels = []
        return self

    def __exit__(self, *exc):
        lib = load_library()
        buf = ctypes.create_string_buffer(1 << 16)
        need = lib.gpuntt_test_launch_log_take(buf, len(buf))
        if need > len(buf):  # nothing was copied and the log was kept: take it again with the room it needs
            buf = ctypes.create_string_buffer(need)
            need = lib.gpuntt_test_launch_log_take(buf, len(buf))
        assert 0 < need <= len(buf), "launch log of %d bytes does not fit %d" % (need, len(buf))
        self.kernels = buf.value.decode().split()
        assert need == len(buf.value) + 1, "launch log cut: %d bytes of %d" % (len(buf.value) + 1, need)
        return False


def _check(rc):
    if rc == GPUNTT_OK:
        return
    msg = load_library().gpuntt_last_error().decode()
    if rc == _ERR_INVALID:
        raise ValueError(msg)  # std::invalid_argument
    raise GpuNttError(msg)


def _bits_of(dtype):
    return {"u32": 32, "s32": 32, "u64": 64, "s64": 64}[dtype]


def _ct(bits):
    return ctypes.c_uint32 if bits == 32 else ctypes.c_uint64


def np_dtype(bits):
    return np.uint32 if bits == 32 else np.uint64


# ------------------------------------------------------------------------------ structs
@dataclass
class Modulus:
    """Modulus<T>{value, bit, mu} (reference modular_arith.cuh:28-57)."""
    value: int
    bit: int = 0
    mu: int = 0
    bits: int = 64

    def __post_init__(self):
        if self.bit == 0:
            lib = load_library()
            m = _M32() if self.bits == 32 else _M64()
            fn = lib.gpuntt_modulus_u32 if self.bits == 32 else lib.gpuntt_modulus_u64
            _check(fn(_ct(self.bits)(self.value), ctypes.byref(m)))
            self.bit, self.mu = int(m.bit), int(m.mu)

    def c(self):
        return (_M32 if self.bits == 32 else _M64)(self.value, self.bit, self.mu)

    def words(self):
        return [self.value, self.bit, self.mu]


@dataclass
class ntt_configuration:
    """reference ntt.cuh:31-40; mod_inverse is a host value."""
    n_power: int
    ntt_type: int = FORWARD
    ntt_layout: int = PerPolynomial
    reduction_poly: int = X_N_minus
    zero_padding: bool = False
    mod_inverse: int = 0
    stream: Optional[object] = None


@dataclass
class ntt_rns_configuration:
    """reference ntt.cuh:42-51; mod_inverse is a device tensor (one word per modulus)."""
    n_power: int
    ntt_type: int = FORWARD
    ntt_layout: int = PerPolynomial
    reduction_poly: int = X_N_minus
    zero_padding: bool = False
    mod_inverse: Optional[object] = None
    stream: Optional[object] = None


@dataclass
class ntt4step_configuration:
    """reference ntt_4step.cuh:19-25"""
    n_power: int
    ntt_type: int = FORWARD
    mod_inverse: int = 0
    stream: Optional[object] = None


@dataclass
class ntt4step_rns_configuration:
    """reference ntt_4step.cuh:27-33"""
    n_power: int
    ntt_type: int = FORWARD
    mod_inverse: Optional[object] = None
    stream: Optional[object] = None


# --------------------------------------------------------------- host-side parameters
class NTTParameters:
    """NTTParameters<T> (reference nttparameters.cuh:56-104) generated by the library's own
    host code; tables are exposed in DEVICE (bit-reversed) order as numpy arrays."""

    def __init__(self, logn, poly_reduction, bits=64, factors=None):
        lib = load_library()
        T = _ct(bits)
        self.bits, self.logn, self.n, self.poly_reduction = bits, logn, 1 << logn, poly_reduction
        size = (1 << (logn - 1)) if poly_reduction == X_N_minus else (1 << logn)
        info = (ctypes.c_uint64 * 8)()
        fwd = np.empty(size, dtype=np_dtype(bits))
        inv = np.empty(size, dtype=np_dtype(bits))
        fac = (T * 3)(*factors) if factors is not None else None
        fn = getattr(lib, "gpuntt_merge_params_u%d" % bits)
        _check(fn(logn, poly_reduction, fac, info, fwd.ctypes.data_as(ctypes.c_void_p),
                  inv.ctypes.data_as(ctypes.c_void_p)))
        self.modulus = Modulus(int(info[0]), int(info[1]), int(info[2]), bits)
        self.omega, self.psi, self.n_inv = int(info[3]), int(info[4]), int(info[5])
        self.root_of_unity_size = int(info[6])
        self.forward_table_device_order = fwd
        self.inverse_table_device_order = inv


class NTTParameters4Step:
    """NTTParameters4Step<T> (reference nttparameters.cuh:106-170)."""

    def __init__(self, logn, bits=64):
        lib = load_library()
        self.bits, self.logn, self.n = bits, logn, 1 << logn
        fn = getattr(lib, "gpuntt_4step_params_u%d" % bits)
        info = (ctypes.c_uint64 * 9)()
        _check(fn(logn, 0, info, None, None, None))
        self.modulus = Modulus(int(info[0]), int(info[1]), int(info[2]), bits)
        self.omega, self.psi, self.n_inv = int(info[3]), int(info[4]), int(info[5])
        self.n1, self.n2 = int(info[6]), int(info[7])
        self.tables = {}
        for inverse, tag in ((0, "fwd"), (1, "inv")):
            t1 = np.empty(self.n1 >> 1, dtype=np_dtype(bits))
            t2 = np.empty(self.n2 >> 1, dtype=np_dtype(bits))
            w = np.empty(self.n, dtype=np_dtype(bits))
            _check(fn(logn, inverse, info, t1.ctypes.data_as(ctypes.c_void_p),
                      t2.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p)))
            self.tables[tag] = (t1, t2, w)


# -------------------------------------------------------------------- device plumbing
def to_device(a, device="cuda:0"):
    """numpy unsigned/signed 32/64-bit array -> torch tensor (int32/int64 storage) on GPU."""
    import torch
    a = np.ascontiguousarray(a)
    view = a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)
    return torch.from_numpy(view.copy()).to(device)


def to_host(t, signed=False):
    a = t.detach().cpu().numpy()
    if signed:
        return a
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def modulus_array_to_device(moduli, bits=64, device="cuda:0"):
    """[Modulus...] -> device array of Modulus<T> (3 words each)."""
    words = np.array([w for m in moduli for w in m.words()], dtype=np_dtype(bits))
    return to_device(words, device)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(s):
    if s is None:
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(s, int):
        return ctypes.c_void_p(s)
    return ctypes.c_void_p(s.cuda_stream)


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("gpu-ntt_amd has no CPU path: tensors must live on the GPU")


def _width(t, dtype):
    if dtype is not None:
        return _bits_of(dtype)
    return t.element_size() * 8


# --------------------------------------------------------------------- the operator API
def GPU_NTT(device_in, device_out, root_of_unity_table, modulus, cfg, batch_size,
            mod_count=None, dtype=None):
    """Forward Merge NTT, natural order in -> bit-reversed out.  `modulus` is a Modulus
    (single-modulus overload, ntt.cuh:315-321) or a device tensor of Modulus<T> words with
    `mod_count` (RNS overload, ntt.cuh:395-401).  dtype 's32'/'s64' selects the signed-input
    instantiation."""
    lib = load_library()
    _require_gpu(device_in, device_out, root_of_unity_table)
    bits = _width(device_out, dtype)
    signed = int(dtype in ("s32", "s64"))
    if isinstance(modulus, Modulus):
        fn = getattr(lib, "gpuntt_ntt_u%d" % bits)
        _check(fn(_ptr(device_in), _ptr(device_out), _ptr(root_of_unity_table), modulus.c(),
                  cfg.n_power, cfg.ntt_layout, cfg.reduction_poly, signed, _stream(cfg.stream),
                  batch_size))
    else:
        _require_gpu(modulus)
        fn = getattr(lib, "gpuntt_ntt_rns_u%d" % bits)
        _check(fn(_ptr(device_in), _ptr(device_out), _ptr(root_of_unity_table), _ptr(modulus),
                  cfg.n_power, cfg.ntt_layout, cfg.reduction_poly, signed, _stream(cfg.stream),
                  batch_size, int(mod_count)))


def GPU_INTT(device_in, device_out, root_of_unity_table, modulus, cfg, batch_size,
             mod_count=None, dtype=None):
    """Inverse Merge NTT, bit-reversed in -> natural out, scaled by cfg.mod_inverse.
    dtype 's32'/'s64' selects the centred signed-output instantiation."""
    lib = load_library()
    _require_gpu(device_in, device_out, root_of_unity_table)
    bits = _width(device_in, dtype)
    signed = int(dtype in ("s32", "s64"))
    if isinstance(modulus, Modulus):
        fn = getattr(lib, "gpuntt_intt_u%d" % bits)
        _check(fn(_ptr(device_in), _ptr(device_out), _ptr(root_of_unity_table), modulus.c(),
                  cfg.n_power, cfg.ntt_layout, cfg.reduction_poly, _ct(bits)(cfg.mod_inverse),
                  signed, _stream(cfg.stream), batch_size))
    else:
        _require_gpu(modulus, cfg.mod_inverse)
        fn = getattr(lib, "gpuntt_intt_rns_u%d" % bits)
        _check(fn(_ptr(device_in), _ptr(device_out), _ptr(root_of_unity_table), _ptr(modulus),
                  cfg.n_power, cfg.ntt_layout, cfg.reduction_poly, _ptr(cfg.mod_inverse), signed,
                  _stream(cfg.stream), batch_size, int(mod_count)))


def GPU_NTT_Inplace(device_inout, root_of_unity_table, modulus, cfg, batch_size, mod_count=None):
    GPU_NTT(device_inout, device_inout, root_of_unity_table, modulus, cfg, batch_size, mod_count)


def GPU_INTT_Inplace(device_inout, root_of_unity_table, modulus, cfg, batch_size, mod_count=None):
    GPU_INTT(device_inout, device_inout, root_of_unity_table, modulus, cfg, batch_size, mod_count)


def _ordered(fname, device_in, device_out, root_of_unity_table, modulus, cfg, batch_size, mod_count, order):
    lib = load_library()
    _require_gpu(device_in, device_out, root_of_unity_table, modulus, order)
    bits = device_in.element_size() * 8
    fn = getattr(lib, "gpuntt_%s_u%d" % (fname, bits))
    _check(fn(_ptr(device_in), _ptr(device_out), _ptr(root_of_unity_table), _ptr(modulus), cfg.n_power,
              cfg.ntt_type, cfg.reduction_poly, _ptr(cfg.mod_inverse), _stream(cfg.stream), batch_size,
              int(mod_count), _ptr(order)))


def GPU_NTT_Modulus_Ordered(device_in, device_out, root_of_unity_table, modulus, cfg, batch_size,
                            mod_count, order):
    """polynomial p uses prime order[p % mod_count] (reference ntt.cuh:515-529); cfg.ntt_type picks
    FORWARD / INVERSE; `order` is an int32 device tensor."""
    _ordered("ntt_modulus_ordered", device_in, device_out, root_of_unity_table, modulus, cfg,
             batch_size, mod_count, order)


def GPU_NTT_Poly_Ordered(device_in, device_out, root_of_unity_table, modulus, cfg, batch_size,
                         mod_count, order):
    """polynomial p is the one in slot order[p] and uses modulus p % mod_count
    (reference ntt.cuh:589-603)."""
    _ordered("ntt_poly_ordered", device_in, device_out, root_of_unity_table, modulus, cfg, batch_size,
             mod_count, order)


def GPU_Transpose(polynomial_in, polynomial_out, row, col, n_power, batch_size):
    """per polynomial (row x col) -> (col x row); default stream (ntt_4step.cuh:46-49)."""
    lib = load_library()
    _require_gpu(polynomial_in, polynomial_out)
    bits = polynomial_in.element_size() * 8
    fn = getattr(lib, "gpuntt_transpose_u%d" % bits)
    _check(fn(_ptr(polynomial_in), _ptr(polynomial_out), row, col, n_power, batch_size))


def GPU_4STEP_NTT(device_in, device_out, n1_root_of_unity_table, n2_root_of_unity_table,
                  W_root_of_unity_table, modulus, cfg, batch_size, mod_count=None):
    """4-step transform of an already transposed (n2 x n1) input into an (n1 x n2) output
    (ntt_4step.cuh:278-308); cfg.ntt_type selects FORWARD / INVERSE."""
    lib = load_library()
    _require_gpu(device_in, device_out, n1_root_of_unity_table, n2_root_of_unity_table,
                 W_root_of_unity_table)
    bits = device_in.element_size() * 8
    if isinstance(modulus, Modulus):
        fn = getattr(lib, "gpuntt_4step_u%d" % bits)
        _check(fn(_ptr(device_in), _ptr(device_out), _ptr(n1_root_of_unity_table),
                  _ptr(n2_root_of_unity_table), _ptr(W_root_of_unity_table), modulus.c(),
                  cfg.n_power, cfg.ntt_type, _ct(bits)(cfg.mod_inverse), _stream(cfg.stream),
                  batch_size))
    else:
        fn = getattr(lib, "gpuntt_4step_rns_u%d" % bits)
        _check(fn(_ptr(device_in), _ptr(device_out), _ptr(n1_root_of_unity_table),
                  _ptr(n2_root_of_unity_table), _ptr(W_root_of_unity_table), _ptr(modulus),
                  cfg.n_power, cfg.ntt_type, _ptr(cfg.mod_inverse), _stream(cfg.stream),
                  batch_size, int(mod_count)))


def GPU_PolyMul(device_a, device_b, device_out, forward_table, inverse_table, modulus, cfg, batch_size,
                mod_count=None):
    """Extension: device_out = INTT(NTT(a) (.) NTT(b)) -- the product in Z_q[X]/(X^N -+ 1) that the
    reference's CPU example builds from NTTCPU::ntt / mult / intt.  a and b are overwritten with their
    transforms; cfg carries n_power, reduction_poly, mod_inverse (N^-1; device array for RNS), stream."""
    lib = load_library()
    _require_gpu(device_a, device_b, device_out, forward_table, inverse_table)
    bits = device_a.element_size() * 8
    if isinstance(modulus, Modulus):
        fn = getattr(lib, "gpuntt_polymul_u%d" % bits)
        _check(fn(_ptr(device_a), _ptr(device_b), _ptr(device_out), _ptr(forward_table), _ptr(inverse_table),
                  modulus.c(), cfg.n_power, cfg.reduction_poly, _ct(bits)(cfg.mod_inverse),
                  _stream(cfg.stream), batch_size))
    else:
        fn = getattr(lib, "gpuntt_polymul_rns_u%d" % bits)
        _check(fn(_ptr(device_a), _ptr(device_b), _ptr(device_out), _ptr(forward_table), _ptr(inverse_table),
                  _ptr(modulus), cfg.n_power, cfg.reduction_poly, _ptr(cfg.mod_inverse), _stream(cfg.stream),
                  batch_size, int(mod_count)))


DOMAIN_NTT, DOMAIN_COEFFICIENT = 0, 1  # gpuntt_automorphism_index_map


def _galois_elts(galois_elts):
    vals = [galois_elts] if isinstance(galois_elts, int) else list(galois_elts)
    if not all(isinstance(e, (int, np.integer)) and 0 <= int(e) < (1 << 32) for e in vals):
        raise ValueError("Galois elements must be 32-bit unsigned integers")
    return (ctypes.c_uint32 * max(1, len(vals)))(*[int(e) for e in vals]), len(vals)


def _check_sizes(device_in, device_out, count, n_power, batch_size):
    """the library cannot see tensor sizes: in must hold batch x N words, out count x batch x N"""
    if 1 <= int(n_power) <= 28 and int(batch_size) > 0:
        words = int(batch_size) << int(n_power)
        if device_in.numel() < words or device_out.numel() < count * words:
            raise ValueError("device_in needs %d words and device_out %d (galois_count x batch x N); got %d and %d"
                             % (words, count * words, device_in.numel(), device_out.numel()))


def GPU_Automorphism_NTT(device_in, device_out, galois_elts, n_power, reduction_poly, batch_size, stream=None):
    """Extension (include/gpuntt/ntt_merge/galois.cuh): sigma_k for every odd k in galois_elts (an int or up to 64 of
    them) applied to polynomials in GPU_NTT's output order -- a permutation, no modulus.  device_in holds batch x N
    words, device_out len(galois_elts) x batch x N; the two must not overlap.  One kernel launch."""
    _require_gpu(device_in, device_out)
    arr, count = _galois_elts(galois_elts)
    _check_sizes(device_in, device_out, count, n_power, batch_size)
    fn = getattr(load_library(), "gpuntt_automorphism_ntt_u%d" % (device_in.element_size() * 8))
    _check(fn(_ptr(device_in), _ptr(device_out), arr, count, int(n_power), int(reduction_poly), _stream(stream),
              int(batch_size)))


def GPU_Automorphism(device_in, device_out, galois_elts, modulus, n_power, reduction_poly, batch_size,
                     mod_count=None, stream=None):
    """Extension: sigma_k in the coefficient domain (negacyclic sign q - x for X_N_plus).  `modulus` is a Modulus or a
    device tensor of Modulus<T> words with `mod_count` (RNS: polynomial p uses modulus p % mod_count).  Layout and
    element rules as GPU_Automorphism_NTT."""
    _require_gpu(device_in, device_out)
    arr, count = _galois_elts(galois_elts)
    _check_sizes(device_in, device_out, count, n_power, batch_size)
    lib = load_library()
    bits = device_in.element_size() * 8
    if isinstance(modulus, Modulus):
        fn = getattr(lib, "gpuntt_automorphism_u%d" % bits)
        _check(fn(_ptr(device_in), _ptr(device_out), arr, count, modulus.c(), int(n_power), int(reduction_poly),
                  _stream(stream), int(batch_size)))
    else:
        _require_gpu(modulus)
        fn = getattr(lib, "gpuntt_automorphism_rns_u%d" % bits)
        _check(fn(_ptr(device_in), _ptr(device_out), arr, count, _ptr(modulus), int(n_power), int(reduction_poly),
                  _stream(stream), int(batch_size), int(mod_count)))


def galois_element_for_rotation(steps, n_power):
    """GaloisElementForRotation: 5^steps mod 2N (negative steps: the inverse)."""
    out = ctypes.c_uint32()
    _check(load_library().gpuntt_galois_element_u32(int(steps), int(n_power), 0, ctypes.byref(out)))
    return int(out.value)


def galois_element_for_conjugation(n_power):
    """GaloisElementForConjugation: 2N - 1."""
    out = ctypes.c_uint32()
    _check(load_library().gpuntt_galois_element_u32(0, int(n_power), 1, ctypes.byref(out)))
    return int(out.value)


def automorphism_index_map(n_power, galois_elt, reduction_poly, domain=DOMAIN_NTT):
    """Host (no GPU): uint32 array of N entries, the source the kernels read for every output slot (DOMAIN_NTT) or
    coefficient (DOMAIN_COEFFICIENT; for X_N_plus an entry j >= N means -in[j - N])."""
    if not 1 <= int(n_power) <= 28:
        raise ValueError("Invalid n_power range!")
    out = np.empty(1 << int(n_power), dtype=np.uint32)
    _check(load_library().gpuntt_automorphism_index_map(int(n_power), ctypes.c_uint32(int(galois_elt) & 0xFFFFFFFF),
                                                        int(reduction_poly), int(domain),
                                                        out.ctypes.data_as(ctypes.c_void_p)))
    return out


def GPU_4STEP_NTT_NaturalOrder(device_in, device_out, n1_root_of_unity_table, n2_root_of_unity_table,
                               W_root_of_unity_table, modulus, cfg, batch_size):
    """Extension: natural-order input -> NTT_4STEP_CPU::ntt / ::intt order in one call (what the
    reference's examples do with GPU_Transpose -> GPU_4STEP_NTT -> GPU_Transpose).  device_in is
    overwritten; device_in is not device_out."""
    lib = load_library()
    _require_gpu(device_in, device_out, n1_root_of_unity_table, n2_root_of_unity_table,
                 W_root_of_unity_table)
    bits = device_in.element_size() * 8
    fn = getattr(lib, "gpuntt_4step_natural_u%d" % bits)
    _check(fn(_ptr(device_in), _ptr(device_out), _ptr(n1_root_of_unity_table),
              _ptr(n2_root_of_unity_table), _ptr(W_root_of_unity_table), modulus.c(), cfg.n_power,
              cfg.ntt_type, _ct(bits)(cfg.mod_inverse), _stream(cfg.stream), batch_size))


class NTTPlan:
    """Extension NTTPlan<T> (include/gpuntt/ntt_merge/ntt.cuh): twiddles prepared once into a workspace;
    execute() launches the transform kernels only (no allocation, synchronisation or preparation).
    `moduli` is a Modulus or a list of Modulus (RNS: polynomial p uses modulus p % len); `mod_inverse`
    an int or list of ints (inverse plans); `workspace` an optional uint8 device tensor of
    workspace_bytes() bytes owned by the caller."""

    def __init__(self, table_device, moduli, n_power, reduction_poly=X_N_minus, ntt_type=FORWARD,
                 mod_inverse=None, batch_hint=1024, stream=None, workspace=None):
        lib = load_library()
        _require_gpu(table_device)
        moduli = [moduli] if isinstance(moduli, Modulus) else list(moduli)
        self.bits = moduli[0].bits
        self.n_power, self.ntt_type, self.mod_count = n_power, ntt_type, len(moduli)
        T = _ct(self.bits)
        marr = ((_M32 if self.bits == 32 else _M64) * len(moduli))(*[m.c() for m in moduli])
        ninv = None
        if mod_inverse is not None:
            vals = [mod_inverse] if isinstance(mod_inverse, int) else list(mod_inverse)
            ninv = (T * len(vals))(*vals)
        self._keep = (table_device, workspace)
        self._h = ctypes.c_void_p()
        fn = getattr(lib, "gpuntt_plan_create_u%d" % self.bits)
        _check(fn(ctypes.byref(self._h), _ptr(table_device), marr, len(moduli), n_power, reduction_poly,
                  ntt_type, ninv, int(batch_hint), _ptr(workspace), _stream(stream)))

    @staticmethod
    def workspace_bytes(n_power, mod_count=1, bits=64):
        lib = load_library()
        out = ctypes.c_uint64()
        _check(getattr(lib, "gpuntt_plan_workspace_bytes_u%d" % bits)(n_power, mod_count, ctypes.byref(out)))
        return int(out.value)

    @property
    def fast_path(self):
        return bool(getattr(load_library(), "gpuntt_plan_fast_path_u%d" % self.bits)(self._h))

    def execute(self, device_in, device_out, batch_size, stream=None, io_signed=False):
        _require_gpu(device_in, device_out)
        fn = getattr(load_library(), "gpuntt_plan_execute_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_in), _ptr(device_out), int(batch_size), int(io_signed), _stream(stream)))

    def close(self):
        if self._h:
            getattr(load_library(), "gpuntt_plan_destroy_u%d" % self.bits)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


APPROXIMATE, CENTRED = 0, 1  # BaseConvMode
BASECONV_TILE = 128  # columns per workgroup of the base conversion kernel (kern::BC_NT)


def _baseconv_moduli(moduli, bits):
    """ints or Modulus objects -> (list of Modulus, C array); a value Modulus<T> refuses raises ValueError"""
    ms = [m if isinstance(m, Modulus) else Modulus(int(m), bits=bits) for m in moduli]
    if any(m.bits != bits for m in ms):
        raise ValueError("every modulus of a BaseConvPlan has the plan's word width")
    return ms, ((_M32 if bits == 32 else _M64) * max(1, len(ms)))(*[m.c() for m in ms])


def baseconv_constants(in_moduli, out_moduli, bits=64):
    """Host (no GPU): the constants a BaseConvPlan of these bases uploads, as a dict of numpy arrays -- qhat_inv[L],
    qhat_inv_shoup[L], matrix[L][K] (qhat_i mod p_j), q_mod_p[K], q_inv_mod_p[K], recip[L] (floor(2^(W-1+b_i) / q_i)
    mod 2^W), bit_length[L].  Raises ValueError where the plan's constructor would."""
    qs, qarr = _baseconv_moduli(in_moduli, bits)
    ps, parr = _baseconv_moduli(out_moduli, bits)
    L, K, dt = len(qs), len(ps), np_dtype(bits)
    shapes = (("qhat_inv", (L,)), ("qhat_inv_shoup", (L,)), ("matrix", (L, K)), ("q_mod_p", (K,)),
              ("q_inv_mod_p", (K,)), ("recip", (L,)), ("bit_length", (L,)))
    out = {name: np.zeros(tuple(max(1, d) for d in shape), dtype=dt) for name, shape in shapes}
    fn = getattr(load_library(), "gpuntt_baseconv_constants_u%d" % bits)
    _check(fn(qarr, L, parr, K, *[out[name].ctypes.data_as(ctypes.c_void_p) for name, _ in shapes]))
    return out


class BaseConvPlan:
    """Extension BaseConvPlan<T> (include/gpuntt/rns/base_conversion.cuh): RNS fast base conversion from the base
    `in_moduli` (q_0 .. q_{L-1}) to the base `out_moduli` (p_0 .. p_{K-1}); ints or Modulus objects, 1 <= L, K <= 64.
    The constants are derived once, on the host, into `workspace` (an optional uint8 device tensor of
    workspace_bytes() bytes owned by the caller).  convert() and convert_and_divide() launch one kernel each and
    allocate nothing.  device_in holds count x L x N words, device_out and device_c count x K x N; device_out may be
    device_c, and must not overlap device_in."""

    def __init__(self, in_moduli, out_moduli, bits=64, stream=None, workspace=None):
        lib = load_library()
        qs, qarr = _baseconv_moduli(in_moduli, bits)
        ps, parr = _baseconv_moduli(out_moduli, bits)
        _require_gpu(workspace)
        self.bits, self.in_count, self.out_count = bits, len(qs), len(ps)
        if workspace is not None and 1 <= len(qs) <= 64 and 1 <= len(ps) <= 64 and \
                workspace.numel() * workspace.element_size() < self.workspace_bytes(len(qs), len(ps), bits):
            raise ValueError("workspace holds fewer than workspace_bytes() bytes")
        self._keep = workspace
        self._h = ctypes.c_void_p()
        fn = getattr(lib, "gpuntt_baseconv_plan_create_u%d" % bits)
        _check(fn(ctypes.byref(self._h), qarr, len(qs), parr, len(ps), _ptr(workspace), _stream(stream)))

    @staticmethod
    def workspace_bytes(in_count, out_count, bits=64):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_baseconv_plan_workspace_bytes_u%d" % bits)(
            int(in_count), int(out_count), ctypes.byref(out)))
        return int(out.value)

    @property
    def owns_workspace(self):
        """False: the plan lives in the caller's workspace and has allocated no device memory"""
        return bool(getattr(load_library(), "gpuntt_baseconv_plan_owns_workspace_u%d" % self.bits)(self._h))

    def _check_buffers(self, device_in, outs, n_power, count):
        """the library cannot see tensor sizes or types"""
        _require_gpu(device_in, *outs)
        if not 1 <= int(n_power) <= 28:
            raise ValueError("Invalid n_power range!")
        for t in (device_in, *outs):
            if t.element_size() * 8 != self.bits or t.dtype.is_floating_point:
                raise ValueError("a %d-bit BaseConvPlan takes %d-bit integer tensors" % (self.bits, self.bits))
        if int(count) > 0:
            words = int(count) << int(n_power)
            if device_in.numel() < self.in_count * words or any(t.numel() < self.out_count * words for t in outs):
                raise ValueError("device_in needs %d words (count x L x N), device_out and device_c %d (count x K x N)"
                                 % (self.in_count * words, self.out_count * words))

    def convert(self, device_in, device_out, n_power, count, mode=CENTRED, stream=None):
        self._check_buffers(device_in, (device_out,), n_power, count)
        fn = getattr(load_library(), "gpuntt_baseconv_plan_convert_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_in), _ptr(device_out), int(n_power), int(count), int(mode), _stream(stream)))

    def convert_and_divide(self, device_in, device_c, device_out, n_power, count, mode=CENTRED, stream=None):
        self._check_buffers(device_in, (device_c, device_out), n_power, count)
        fn = getattr(load_library(), "gpuntt_baseconv_plan_convert_and_divide_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_in), _ptr(device_c), _ptr(device_out), int(n_power), int(count), int(mode),
                  _stream(stream)))

    def close(self):
        if self._h:
            getattr(load_library(), "gpuntt_baseconv_plan_destroy_u%d" % self.bits)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _innerprod_moduli(moduli, bits):
    """ints or Modulus objects -> (list of Modulus, C array); a value Modulus<T> refuses raises ValueError"""
    ms = [m if isinstance(m, Modulus) else Modulus(int(m), bits=bits) for m in moduli]
    if any(m.bits != bits for m in ms):
        raise ValueError("every modulus of an InnerProductPlan has the plan's word width")
    return ms, ((_M32 if bits == 32 else _M64) * max(1, len(ms)))(*[m.c() for m in ms])


def _innerprod_limbs(key_limbs, mod_count):
    """None (the identity) or mod_count ints -> a C int array or None"""
    if key_limbs is None:
        return None
    limbs = [int(v) for v in key_limbs]
    if len(limbs) != mod_count:
        raise ValueError("key_limbs holds one key limb index per modulus of the plan")
    return (ctypes.c_int * max(1, len(limbs)))(*limbs)


def innerprod_constants(moduli, bits=64):
    """Host (no GPU): the folding constants an InnerProductPlan of these moduli uploads, as a dict of numpy arrays of M
    words -- pow_w (2^W mod q), pow_w_shoup, pow_2w (2^2W mod q), pow_2w_shoup, one_shoup (floor(2^W / q)).  Raises
    ValueError where the plan's constructor would."""
    ms, marr = _innerprod_moduli(moduli, bits)
    names = ("pow_w", "pow_w_shoup", "pow_2w", "pow_2w_shoup", "one_shoup")
    out = {name: np.zeros(max(1, len(ms)), dtype=np_dtype(bits)) for name in names}
    fn = getattr(load_library(), "gpuntt_innerprod_constants_u%d" % bits)
    _check(fn(marr, len(ms), *[out[name].ctypes.data_as(ctypes.c_void_p) for name in names]))
    return out


def innerprod_reference(moduli, a, key, out, n_power, digits, components, count, accumulate=False, key_mod_count=None,
                        key_limbs=None, bits=64):
    """Host (no GPU): InnerProductPlan<T>::reference -- the definition of multiply_accumulate on numpy arrays of the
    plan's word type, in exact integers, after the argument checks of the call itself (ValueError).  `out` is written
    in place (and read first when accumulating) and returned.  None for an array is the C NULL."""
    ms, marr = _innerprod_moduli(moduli, bits)
    M, dt = len(ms), np_dtype(bits)
    km = M if key_mod_count is None else int(key_mod_count)
    limbs = _innerprod_limbs(key_limbs, M)
    need = None
    if 1 <= int(n_power) <= 28 and int(count) >= 0 and int(digits) >= 1 and int(components) >= 1 and km >= 1:
        words = (int(count) * M) << int(n_power)
        need = (int(digits) * words, (int(digits) * int(components) * km) << int(n_power), int(components) * words)
    for i, arr in enumerate((a, key, out)):
        if arr is None:
            continue
        if arr.dtype != dt or not arr.flags["C_CONTIGUOUS"]:
            raise ValueError("innerprod_reference takes C-contiguous %d-bit unsigned arrays" % bits)
        if need is not None and arr.size < need[i]:
            raise ValueError("a needs %d words (D x count x M x N), key %d (D x C x key_mod_count x N), out %d "
                             "(C x count x M x N)" % need)
    ptr = [ctypes.c_void_p(0 if arr is None else arr.ctypes.data) for arr in (a, key, out)]
    fn = getattr(load_library(), "gpuntt_innerprod_reference_u%d" % bits)
    _check(fn(marr, M, ptr[0], ptr[1], ptr[2], int(n_power), int(digits), int(components), int(count),
              1 if accumulate else 0, km, limbs))
    return out


class InnerProductPlan:
    """Extension InnerProductPlan<T> (include/gpuntt/rns/inner_product.cuh): the key-switching multiply-accumulate for
    the moduli q_0 .. q_{M-1} (ints or Modulus objects, 1 <= M <= 64).  The folding constants are derived once, on the
    host, into `workspace` (an optional uint8 device tensor of workspace_bytes() bytes owned by the caller).
    multiply_accumulate() launches one kernel and allocates nothing."""

    def __init__(self, moduli, bits=64, stream=None, workspace=None):
        lib = load_library()
        ms, marr = _innerprod_moduli(moduli, bits)
        _require_gpu(workspace)
        self.bits, self.mod_count = bits, len(ms)
        if workspace is not None and 1 <= len(ms) <= 64 and \
                workspace.numel() * workspace.element_size() < self.workspace_bytes(len(ms), bits):
            raise ValueError("workspace holds fewer than workspace_bytes() bytes")
        self._keep = workspace
        self._h = ctypes.c_void_p()
        fn = getattr(lib, "gpuntt_innerprod_plan_create_u%d" % bits)
        _check(fn(ctypes.byref(self._h), marr, len(ms), _ptr(workspace), _stream(stream)))

    @staticmethod
    def workspace_bytes(mod_count, bits=64):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_innerprod_plan_workspace_bytes_u%d" % bits)(
            int(mod_count), ctypes.byref(out)))
        return int(out.value)

    @property
    def owns_workspace(self):
        """False: the plan lives in the caller's workspace and has allocated no device memory"""
        return bool(getattr(load_library(), "gpuntt_innerprod_plan_owns_workspace_u%d" % self.bits)(self._h))

    def _check_buffers(self, a, key, out, n_power, digits, components, count, key_mod_count):
        """the library cannot see tensor sizes or types"""
        _require_gpu(a, key, out)
        if not 1 <= int(n_power) <= 28:
            raise ValueError("Invalid n_power range!")
        for t in (a, key, out):
            if t.element_size() * 8 != self.bits or t.dtype.is_floating_point:
                raise ValueError("a %d-bit InnerProductPlan takes %d-bit integer tensors" % (self.bits, self.bits))
        if int(count) > 0 and int(digits) >= 1 and int(components) >= 1 and int(key_mod_count) >= 1:
            words = (int(count) * self.mod_count) << int(n_power)
            need = (int(digits) * words, (int(digits) * int(components) * int(key_mod_count)) << int(n_power),
                    int(components) * words)
            if a.numel() < need[0] or key.numel() < need[1] or out.numel() < need[2]:
                raise ValueError("a needs %d words (D x count x M x N), key %d (D x C x key_mod_count x N), out %d "
                                 "(C x count x M x N)" % need)

    def multiply_accumulate(self, a, key, out, n_power, digits, components, count, accumulate=False,
                            key_mod_count=None, key_limbs=None, stream=None):
        """out[c][r][m] (+)= sum_d a[d][r][m] * key[d][c][key_limbs[m]] mod q_m, pointwise over the N columns: a holds
        digits x count x M x N words, key (at least) digits x components x key_mod_count x N, out components x count x
        M x N.  key_mod_count defaults to M, key_limbs (M indices into the key's limbs) to the identity."""
        km = self.mod_count if key_mod_count is None else int(key_mod_count)
        self._check_buffers(a, key, out, n_power, digits, components, count, km)
        limbs = _innerprod_limbs(key_limbs, self.mod_count)
        fn = getattr(load_library(), "gpuntt_innerprod_plan_execute_u%d" % self.bits)
        _check(fn(self._h, _ptr(a), _ptr(key), _ptr(out), int(n_power), int(digits), int(components), int(count),
                  1 if accumulate else 0, km, limbs, _stream(stream)))

    def close(self):
        if self._h:
            getattr(load_library(), "gpuntt_innerprod_plan_destroy_u%d" % self.bits)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _keyswitch_moduli(moduli, bits):
    """ints or Modulus objects -> (list of Modulus, C array); a value Modulus<T> refuses raises ValueError"""
    ms = [m if isinstance(m, Modulus) else Modulus(int(m), bits=bits) for m in moduli]
    if any(m.bits != bits for m in ms):
        raise ValueError("every modulus of a KeySwitchPlan has the plan's word width")
    return ms, ((_M32 if bits == 32 else _M64) * max(1, len(ms)))(*[m.c() for m in ms])


def keyswitch_digits(q_count, alpha):
    """D = ceil(L / alpha)"""
    return -(-int(q_count) // max(1, int(alpha)))


def keyswitch_scratch_bytes(q_count, p_count, alpha, n_power, count, components=1, bits=64):
    """KeySwitchPlan<T>::scratch_bytes (host only): the caller-owned scratch of the pipeline calls, in bytes"""
    out = ctypes.c_uint64()
    _check(getattr(load_library(), "gpuntt_keyswitch_plan_scratch_bytes_u%d" % bits)(
        int(q_count), int(p_count), int(alpha), int(n_power), int(count), int(components), ctypes.byref(out)))
    return int(out.value)


def keyswitch_hoisted_scratch_bytes(q_count, p_count, alpha, n_power, count, elements, bits=64):
    """KeySwitchPlan<T>::hoisted_scratch_bytes (host only): the caller-owned scratch of rotate_hoisted, in bytes -- the
    accumulators T[elements][2][count][M][N], rounded up to 256"""
    out = ctypes.c_uint64()
    _check(getattr(load_library(), "gpuntt_keyswitch_plan_hoisted_scratch_bytes_u%d" % bits)(
        int(q_count), int(p_count), int(alpha), int(n_power), int(count), int(elements), ctypes.byref(out)))
    return int(out.value)


def keyswitch_hoist_chunk(bits, digits, n_power):
    """test hook read-back (csrc/test_hooks.h, host only): log2 of the source chunk inner_product_galois takes for this
    word width, digit count and ring under the current value of the hook keyswitch_hoist_chunk"""
    lc = load_library().gpuntt_test_keyswitch_hoist_chunk(int(bits) // 8, int(digits), int(n_power))
    if lc < 0:
        raise ValueError("Invalid argument!")
    return lc


def keyswitch_hoisted_sum_scratch_bytes(q_count, p_count, alpha, n_power, count, bits=64):
    """KeySwitchPlan<T>::hoisted_sum_scratch_bytes (host only): the caller-owned scratch of rotate_hoisted_sum, in bytes
    -- the accumulators T[2][count][M][N], rounded up to 256; it does not depend on the number of elements"""
    out = ctypes.c_uint64()
    _check(getattr(load_library(), "gpuntt_keyswitch_plan_hoisted_sum_scratch_bytes_u%d" % bits)(
        int(q_count), int(p_count), int(alpha), int(n_power), int(count), ctypes.byref(out)))
    return int(out.value)


def keyswitch_hoist_sum_chunk(bits, digits, n_power):
    """test hook read-back (csrc/test_hooks.h, host only): log2 of the destination chunk inner_product_galois_sum takes
    for this word width, digit count and ring under the current value of the hook keyswitch_hoist_chunk"""
    lc = load_library().gpuntt_test_keyswitch_hoist_sum_chunk(int(bits) // 8, int(digits), int(n_power))
    if lc < 0:
        raise ValueError("Invalid argument!")
    return lc


def bsgs_sum_shape(bits, n1, n_power, aligned):
    """test hook read-back (csrc/test_hooks.h, host only): the launch shape of bsgs_weighted_sum for this word width, n1
    baby steps and ring -- (V, nt): words per lane (a 16-byte group, or 1) and lanes per workgroup; aligned: every base
    pointer of the launch is 16-byte aligned"""
    V, nt = ctypes.c_int(), ctypes.c_uint()
    if load_library().gpuntt_test_bsgs_sum_shape(int(bits) // 8, int(n1), int(n_power), int(bool(aligned)),
                                                 ctypes.byref(V), ctypes.byref(nt)) != 0:
        raise ValueError("Invalid argument!")
    return int(V.value), int(nt.value)


def keyswitch_constants(q_moduli, p_moduli, alpha, bits=64):
    """Host (no GPU): the constants a KeySwitchPlan of these bases uploads (KeySwitchConstants<T>), as a dict of numpy
    arrays -- per digit the ModUp constants up_qhat_inv[L], up_qhat_inv_shoup[L], up_matrix[L][M], up_q_mod[D][M],
    up_recip[L], up_bit_length[L]; the ModDown constants down_qhat_inv[K], down_qhat_inv_shoup[K], down_matrix[K][L],
    down_p_mod_q[L], down_p_inv_mod_q[L], down_recip[K], down_bit_length[K]; the folding constants pow_w, pow_w_shoup,
    pow_2w, pow_2w_shoup, one_shoup [M].  Raises ValueError where the plan's constructor would."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    ps, parr = _keyswitch_moduli(p_moduli, bits)
    L, K, dt = len(qs), len(ps), np_dtype(bits)
    M, D = L + K, keyswitch_digits(L, alpha)
    shapes = (("up_qhat_inv", (L,)), ("up_qhat_inv_shoup", (L,)), ("up_matrix", (L, M)), ("up_q_mod", (D, M)),
              ("up_recip", (L,)), ("up_bit_length", (L,)), ("down_qhat_inv", (K,)), ("down_qhat_inv_shoup", (K,)),
              ("down_matrix", (K, L)), ("down_p_mod_q", (L,)), ("down_p_inv_mod_q", (L,)), ("down_recip", (K,)),
              ("down_bit_length", (K,)), ("pow_w", (M,)), ("pow_w_shoup", (M,)), ("pow_2w", (M,)),
              ("pow_2w_shoup", (M,)), ("one_shoup", (M,)))
    out = {name: np.zeros(tuple(max(1, d) for d in shape), dtype=dt) for name, shape in shapes}
    ptrs = (ctypes.c_void_p * len(shapes))(*[out[name].ctypes.data for name, _ in shapes])
    fn = getattr(load_library(), "gpuntt_keyswitch_constants_u%d" % bits)
    _check(fn(qarr, L, parr, K, int(alpha), ptrs))
    return out


def _keyswitch_host_array(arr, bits, words, what):
    if arr is None:
        return ctypes.c_void_p(0)
    if arr.dtype != np_dtype(bits) or not arr.flags["C_CONTIGUOUS"]:
        raise ValueError("the key switching references take C-contiguous %d-bit unsigned arrays" % bits)
    if words is not None and arr.size < words:
        raise ValueError("%s needs %d words" % (what, words))
    return ctypes.c_void_p(arr.ctypes.data)


def keyswitch_reference_mod_up(q_moduli, p_moduli, alpha, x, a, n_power, count, mode=CENTRED, bits=64):
    """Host (no GPU): KeySwitchPlan<T>::reference_mod_up on numpy arrays of the plan's word type -- x holds count x L x
    N words, a D x count x M x N (written and returned) -- after the argument checks of mod_up (ValueError).  None for
    an array is the C NULL."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    ps, parr = _keyswitch_moduli(p_moduli, bits)
    L, M = len(qs), len(qs) + len(ps)
    ok = 1 <= int(n_power) <= 28 and int(count) >= 0 and int(alpha) >= 1
    cols = (int(count) << int(n_power)) if ok else None
    px = _keyswitch_host_array(x, bits, cols * L if ok else None, "in (count x L x N)")
    pa = _keyswitch_host_array(a, bits, cols * M * keyswitch_digits(L, alpha) if ok else None, "a (D x count x M x N)")
    fn = getattr(load_library(), "gpuntt_keyswitch_reference_mod_up_u%d" % bits)
    _check(fn(qarr, len(qs), parr, len(ps), int(alpha), px, pa, int(n_power), int(count), int(mode)))
    return a


def keyswitch_reference_mod_down(q_moduli, p_moduli, x, out, n_power, stacks, bits=64):
    """Host (no GPU): KeySwitchPlan<T>::reference_mod_down -- x holds stacks x M x N words, out stacks x L x N (written
    and returned)."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    ps, parr = _keyswitch_moduli(p_moduli, bits)
    L, M = len(qs), len(qs) + len(ps)
    ok = 1 <= int(n_power) <= 28 and int(stacks) >= 0
    cols = (int(stacks) << int(n_power)) if ok else None
    px = _keyswitch_host_array(x, bits, cols * M if ok else None, "x (stacks x M x N)")
    po = _keyswitch_host_array(out, bits, cols * L if ok else None, "out (stacks x L x N)")
    fn = getattr(load_library(), "gpuntt_keyswitch_reference_mod_down_u%d" % bits)
    _check(fn(qarr, len(qs), parr, len(ps), px, po, int(n_power), int(stacks)))
    return out


def keyswitch_reference_mod_down_rescale(q_moduli, p_moduli, rescale_limbs, x, out, n_power, stacks, bits=64):
    """Host (no GPU): KeySwitchPlan<T>::reference_mod_down_rescale -- x holds stacks x M x N words, out stacks x (L - R)
    x N (written and returned), R = rescale_limbs in [1, L - 1] (ValueError otherwise)."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    ps, parr = _keyswitch_moduli(p_moduli, bits)
    L, M, R = len(qs), len(qs) + len(ps), int(rescale_limbs)
    ok = 1 <= int(n_power) <= 28 and int(stacks) >= 0 and 1 <= R <= L - 1
    cols = (int(stacks) << int(n_power)) if ok else None
    px = _keyswitch_host_array(x, bits, cols * M if ok else None, "x (stacks x M x N)")
    po = _keyswitch_host_array(out, bits, cols * (L - R) if ok else None, "out (stacks x (L - R) x N)")
    fn = getattr(load_library(), "gpuntt_keyswitch_reference_mod_down_rescale_u%d" % bits)
    _check(fn(qarr, len(qs), parr, len(ps), R, px, po, int(n_power), int(stacks)))
    return out


def keyswitch_reference_rescale(q_moduli, rescale_limbs, x, out, n_power, stacks, bits=64):
    """Host (no GPU): KeySwitchPlan<T>::reference_rescale, coefficient form -- x holds stacks x L x N words over the
    q-base, out stacks x (L - R) x N (written and returned), R = rescale_limbs in [1, L - 1] (ValueError otherwise)."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    L, R = len(qs), int(rescale_limbs)
    ok = 1 <= int(n_power) <= 28 and int(stacks) >= 0 and 1 <= R <= L - 1
    cols = (int(stacks) << int(n_power)) if ok else None
    px = _keyswitch_host_array(x, bits, cols * L if ok else None, "x (stacks x L x N)")
    po = _keyswitch_host_array(out, bits, cols * (L - R) if ok else None, "out (stacks x (L - R) x N)")
    fn = getattr(load_library(), "gpuntt_keyswitch_reference_rescale_u%d" % bits)
    _check(fn(qarr, len(qs), R, px, po, int(n_power), int(stacks)))
    return out


class KeySwitchPlan:
    """Extension KeySwitchPlan<T> (include/gpuntt/rns/key_switch.cuh): hybrid key switching for the q-base `q_moduli`
    (L), the special primes `p_moduli` (K) and the digit size `alpha` on a ring of 2^n_power, M = L + K <= 64.
    forward_table / inverse_table: device tensors as for GPU_NTT / GPU_INTT over the full base (slot i at i << n_power),
    mod_inverse the M host n^-1 values; all three None: a plan without transforms (mod_up / mod_down only).
    key_mod_count / key_limbs as for InnerProductPlan.multiply_accumulate.  `workspace`: an optional uint8 device
    tensor of workspace_bytes() bytes owned by the caller.  `scratch` of the pipeline calls: a device tensor of at least
    plan.scratch_bytes(count, components) bytes -- the header's static scratch_bytes(L, K, alpha, n_power, count,
    components) with this plan's shape filled in; keyswitch_scratch_bytes() is that static -- 256-byte aligned, owned by
    the caller; nothing is allocated by any call.  `rescale_limbs` = R in [0, L - 1]: with R > 0 the plan also holds what
    mod_down_rescale, rescale and the three *_rescale pipeline calls need (workspace_bytes(..., rescale_limbs=R) bytes);
    with R = 0 it is the plan without the argument and those calls raise ValueError."""

    def __init__(self, q_moduli, p_moduli, alpha, n_power, forward_table=None, inverse_table=None, mod_inverse=None,
                 reduction_poly=X_N_plus, batch_hint=1024, key_mod_count=None, key_limbs=None, bits=64, stream=None,
                 workspace=None, rescale_limbs=0, via_rescale_abi=None):
        lib = load_library()
        qs, qarr = _keyswitch_moduli(q_moduli, bits)
        ps, parr = _keyswitch_moduli(p_moduli, bits)
        _require_gpu(workspace, forward_table, inverse_table)
        self.bits, self.q_count, self.p_count, self.mod_count = bits, len(qs), len(ps), len(qs) + len(ps)
        self.alpha, self.n_power = int(alpha), int(n_power)
        self._rescale_limbs = int(rescale_limbs)
        self.kept_count = self.q_count - self._rescale_limbs  # L' = L - R
        # R = 0 goes through gpuntt_keyswitch_plan_create_* unless via_rescale_abi asks for the _rescale_ function
        rescale_abi = self._rescale_limbs != 0 if via_rescale_abi is None else bool(via_rescale_abi)
        self.digits = keyswitch_digits(len(qs), alpha)
        for t in (forward_table, inverse_table):
            if t is not None and (t.element_size() * 8 != bits or t.numel() < self.mod_count << self.n_power):
                raise ValueError("a table holds M x N %d-bit words" % bits)
        ninv = None
        if mod_inverse is not None:
            vals = [int(v) for v in mod_inverse]
            if len(vals) != self.mod_count:
                raise ValueError("mod_inverse holds one n^-1 per modulus of the full base")
            ninv = (_ct(bits) * max(1, len(vals)))(*vals)
        km = self.mod_count if key_mod_count is None else int(key_mod_count)
        limbs = _innerprod_limbs(key_limbs, self.mod_count)
        if workspace is not None:
            # raises for counts out of range
            need = self.workspace_bytes(len(qs), len(ps), alpha, n_power, bits, self._rescale_limbs)
            if workspace.numel() * workspace.element_size() < need:
                raise ValueError("workspace holds fewer than workspace_bytes() bytes")
        self.key_mod_count = km
        self._keep = (workspace, forward_table, inverse_table)
        self._h = ctypes.c_void_p()
        head = (ctypes.byref(self._h), qarr, len(qs), parr, len(ps), int(alpha), int(n_power), _ptr(forward_table),
                _ptr(inverse_table), ninv, int(reduction_poly), int(batch_hint), km, limbs)
        if rescale_abi:
            fn = getattr(lib, "gpuntt_keyswitch_plan_create_rescale_u%d" % bits)
            _check(fn(*head, self._rescale_limbs, _ptr(workspace), _stream(stream)))
        else:
            fn = getattr(lib, "gpuntt_keyswitch_plan_create_u%d" % bits)
            _check(fn(*head, _ptr(workspace), _stream(stream)))

    @staticmethod
    def workspace_bytes(q_count, p_count, alpha, n_power, bits=64, rescale_limbs=0):
        out = ctypes.c_uint64()
        if int(rescale_limbs) != 0:
            _check(getattr(load_library(), "gpuntt_keyswitch_plan_workspace_bytes_rescale_u%d" % bits)(
                int(q_count), int(p_count), int(alpha), int(n_power), int(rescale_limbs), ctypes.byref(out)))
        else:
            _check(getattr(load_library(), "gpuntt_keyswitch_plan_workspace_bytes_u%d" % bits)(
                int(q_count), int(p_count), int(alpha), int(n_power), ctypes.byref(out)))
        return int(out.value)

    @property
    def rescale_limbs(self):
        """R: the q-limbs the *_rescale calls drop (0: the plan has none of them)"""
        return int(getattr(load_library(), "gpuntt_keyswitch_plan_rescale_limbs_u%d" % self.bits)(self._h))

    def scratch_bytes(self, count, components=1):
        return keyswitch_scratch_bytes(self.q_count, self.p_count, self.alpha, self.n_power, count, components,
                                       self.bits)

    @property
    def owns_workspace(self):
        """False: the plan lives in the caller's workspace and has allocated no device memory"""
        return bool(getattr(load_library(), "gpuntt_keyswitch_plan_owns_workspace_u%d" % self.bits)(self._h))

    def _check_buffers(self, sized):
        """the library cannot see tensor sizes or types: sized = (tensor, words needed, name) ..."""
        _require_gpu(*[t for t, _, _ in sized])
        for t, words, name in sized:
            if t.element_size() * 8 != self.bits or t.dtype.is_floating_point:
                raise ValueError("a %d-bit KeySwitchPlan takes %d-bit integer tensors" % (self.bits, self.bits))
            if words > 0 and t.numel() < words:
                raise ValueError("%s needs %d words; got %d" % (name, words, t.numel()))

    def _check_scratch(self, scratch, count, components):
        _require_gpu(scratch)
        if scratch is None:
            raise ValueError("the pipeline calls need a caller-owned scratch of scratch_bytes() bytes")
        if int(count) > 0:
            if scratch.numel() * scratch.element_size() < self.scratch_bytes(count, components):
                raise ValueError("scratch holds fewer than scratch_bytes(count, components) bytes")
            if scratch.data_ptr() % 256:
                raise ValueError("scratch must be 256-byte aligned")

    def _cols(self, count):
        return (int(count) << self.n_power) if int(count) > 0 else 0

    def mod_up(self, device_in, device_a, count, mode=CENTRED, stream=None):
        """device_in T[count][L][N] -> device_a T[D][count][M][N]; one kernel launch"""
        cols = self._cols(count)
        self._check_buffers(((device_in, cols * self.q_count, "in (count x L x N)"),
                             (device_a, cols * self.mod_count * self.digits, "a (D x count x M x N)")))
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_mod_up_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_in), _ptr(device_a), int(count), int(mode), _stream(stream)))

    def mod_down(self, device_x, device_out, stacks, stream=None):
        """device_x T[stacks][M][N] -> device_out T[stacks][L][N]; one kernel launch"""
        cols = self._cols(stacks)
        self._check_buffers(((device_x, cols * self.mod_count, "x (stacks x M x N)"),
                             (device_out, cols * self.q_count, "out (stacks x L x N)")))
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_mod_down_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_x), _ptr(device_out), int(stacks), _stream(stream)))

    def mod_down_add(self, device_x, device_addend, device_out, stacks, stream=None):
        """device_x T[stacks][M][N], device_addend T[stacks][L][N] (any words; it may be device_out itself) ->
        device_out T[stacks][L][N] = (mod_down(x) + addend) mod q; one kernel launch"""
        if device_x is None or device_addend is None or device_out is None:
            raise ValueError("null pointer argument")
        cols = self._cols(stacks)
        self._check_buffers(((device_x, cols * self.mod_count, "x (stacks x M x N)"),
                             (device_addend, cols * self.q_count, "addend (stacks x L x N)"),
                             (device_out, cols * self.q_count, "out (stacks x L x N)")))
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_mod_down_add_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_x), _ptr(device_addend), _ptr(device_out), int(stacks), _stream(stream)))

    def decompose(self, device_c_in, device_a, count, input_ntt=False, scratch=None, stream=None):
        cols = self._cols(count)
        self._check_buffers(((device_c_in, cols * self.q_count, "c_in (count x L x N)"),
                             (device_a, cols * self.mod_count * self.digits, "a (D x count x M x N)")))
        if input_ntt or scratch is not None:
            self._check_scratch(scratch, count, 1)
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_decompose_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_c_in), _ptr(device_a), int(count), int(bool(input_ntt)), _ptr(scratch),
                  _stream(stream)))

    def _key_words(self, components):
        return (self.digits * int(components) * self.key_mod_count) << self.n_power

    def switch_digits(self, device_a, device_key, device_out, count, components, output_ntt=False, scratch=None,
                      stream=None):
        cols = self._cols(count)
        ok = 1 <= int(components) <= 4
        self._check_buffers(((device_a, cols * self.mod_count * self.digits, "a (D x count x M x N)"),
                             (device_key, self._key_words(components) if ok and cols else 0,
                              "key (D x C x key_mod_count x N)"),
                             (device_out, cols * self.q_count * int(components) if ok else 0, "out (C x count x L x N)")))
        if ok:
            self._check_scratch(scratch, count, components)
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_switch_digits_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_a), _ptr(device_key), _ptr(device_out), int(count), int(components),
                  int(bool(output_ntt)), _ptr(scratch), _stream(stream)))

    def apply(self, device_c_in, device_key, device_out, count, components, input_ntt=False, output_ntt=False,
              scratch=None, stream=None):
        cols = self._cols(count)
        ok = 1 <= int(components) <= 4
        self._check_buffers(((device_c_in, cols * self.q_count, "c_in (count x L x N)"),
                             (device_key, self._key_words(components) if ok and cols else 0,
                              "key (D x C x key_mod_count x N)"),
                             (device_out, cols * self.q_count * int(components) if ok else 0, "out (C x count x L x N)")))
        if ok:
            self._check_scratch(scratch, count, components)
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_apply_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_c_in), _ptr(device_key), _ptr(device_out), int(count), int(components),
                  int(bool(input_ntt)), int(bool(output_ntt)), _ptr(scratch), _stream(stream)))

    def hoisted_scratch_bytes(self, count, elements):
        return keyswitch_hoisted_scratch_bytes(self.q_count, self.p_count, self.alpha, self.n_power, count, elements,
                                               self.bits)

    def rotate_hoisted(self, a, c0, keys, elements, out, count, output_ntt=False, scratch=None, stream=None):
        """G = len(elements) Galois automorphisms of one decomposition, each with its own key: a T[D][count][M][N] (what
        decompose writes), c0 T[count][L][N] in NTT form or None, keys a list of G device tensors (each at least
        D x 2 x key_mod_count x N words), elements a list of G odd ints, out T[G][2][count][L][N]; scratch: a device
        tensor of at least hoisted_scratch_bytes(count, G) bytes, 256-byte aligned.  out[g] equals
        GPU_Automorphism_NTT + switch_digits + the rotated c0, word for word (key_switch.cuh)."""
        keys, elements = list(keys), [int(k) for k in elements]
        G, cols = len(elements), self._cols(count)
        if len(keys) != G:
            raise ValueError("rotate_hoisted takes one key per Galois element")
        if not 1 <= G <= 64:
            raise ValueError("Invalid galois_count!")
        if a is None or out is None or scratch is None or any(k is None for k in keys):
            raise ValueError("null pointer argument")
        sized = [(a, cols * self.mod_count * self.digits, "a (D x count x M x N)"),
                 (out, cols * self.q_count * 2 * G, "out (G x 2 x count x L x N)")]
        if c0 is not None:
            sized.append((c0, cols * self.q_count, "c0 (count x L x N)"))
        sized += [(k, self._key_words(2) if cols else 0, "key (D x 2 x key_mod_count x N)") for k in keys]
        self._check_buffers(sized)
        _require_gpu(scratch)
        if int(count) >= 0 and scratch.numel() * scratch.element_size() < self.hoisted_scratch_bytes(count, G):
            raise ValueError("scratch holds fewer than hoisted_scratch_bytes(count, elements) bytes")
        key_ptrs = (ctypes.c_void_p * G)(*[k.data_ptr() for k in keys])
        elts = (ctypes.c_uint32 * G)(*[k & 0xFFFFFFFF for k in elements])
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_rotate_hoisted_u%d" % self.bits)
        _check(fn(self._h, _ptr(a), _ptr(c0), key_ptrs, elts, G, _ptr(out), int(count), int(bool(output_ntt)),
                  _ptr(scratch), _stream(stream)))

    def hoisted_sum_scratch_bytes(self, count):
        return keyswitch_hoisted_sum_scratch_bytes(self.q_count, self.p_count, self.alpha, self.n_power, count,
                                                   self.bits)

    def rotate_hoisted_sum(self, a, c0, keys, elements, weights, out, count, output_ntt=False, scratch=None,
                           stream=None, _rescale=False):
        """The weighted sum of G = len(elements) Galois automorphisms of one decomposition, taken before the ModDown:
        a, c0, keys and elements as for rotate_hoisted; weights None (all 1) or a list of G entries, each None (1) or a
        device tensor of at least M x N words -- the plaintext diagonal in NTT form over the plan's full base; out
        T[2][count][L][N]; scratch: a device tensor of at least hoisted_sum_scratch_bytes(count) bytes, 256-byte
        aligned.  One INTT, one mod_down and one NTT whatever G is; the result rounds once (key_switch.cuh)."""
        keys, elements = list(keys), [int(k) for k in elements]
        G, cols = len(elements), self._cols(count)
        if len(keys) != G:
            raise ValueError("rotate_hoisted_sum takes one key per Galois element")
        weights = None if weights is None else list(weights)
        if weights is not None and len(weights) != G:
            raise ValueError("rotate_hoisted_sum takes one weight (or None) per Galois element")
        if not 1 <= G <= 64:
            raise ValueError("Invalid galois_count!")
        if a is None or out is None or scratch is None or any(k is None for k in keys):
            raise ValueError("null pointer argument")
        sized = [(a, cols * self.mod_count * self.digits, "a (D x count x M x N)"),
                 (out, cols * self._out_limbs(_rescale) * 2, "out (2 x count x L x N)")]
        if c0 is not None:
            sized.append((c0, cols * self.q_count, "c0 (count x L x N)"))
        sized += [(k, self._key_words(2) if cols else 0, "key (D x 2 x key_mod_count x N)") for k in keys]
        sized += [(w, self.mod_count << self.n_power if cols else 0, "weight (M x N)")
                  for w in (weights or ()) if w is not None]
        self._check_buffers(sized)
        _require_gpu(scratch)
        if int(count) >= 0 and scratch.numel() * scratch.element_size() < self.hoisted_sum_scratch_bytes(count):
            raise ValueError("scratch holds fewer than hoisted_sum_scratch_bytes(count) bytes")
        key_ptrs = (ctypes.c_void_p * G)(*[k.data_ptr() for k in keys])
        weight_ptrs = None if weights is None else \
            (ctypes.c_void_p * G)(*[None if w is None else w.data_ptr() for w in weights])
        elts = (ctypes.c_uint32 * G)(*[k & 0xFFFFFFFF for k in elements])
        fn = self._pipeline_fn("rotate_hoisted_sum", _rescale)
        _check(fn(self._h, _ptr(a), _ptr(c0), key_ptrs, elts, weight_ptrs, G, _ptr(out), int(count),
                  int(bool(output_ntt)), _ptr(scratch), _stream(stream)))

    def multiply_relinearize(self, x, y, key, out, count, output_ntt, scratch, stream=None, _rescale=False):
        """The product of `count` pairs of two-component ciphertexts, relinearized in ONE key switch: x, y
        T[2][count][L][N] in NTT form (any words; y may be x), key the relinearization key, at least
        D x 2 x key_mod_count x N words, out T[2][count][L][N] (may be exactly x or exactly y); scratch: a device tensor
        of at least scratch_bytes(count, 2) bytes, 256-byte aligned.  out equals the three pointwise products, apply on
        x1 y1 and the two additions word for word (key_switch.cuh)."""
        if x is None or y is None or key is None or out is None or scratch is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        self._check_buffers(((x, cols * self.q_count * 2, "x (2 x count x L x N)"),
                             (y, cols * self.q_count * 2, "y (2 x count x L x N)"),
                             (key, self._key_words(2) if cols else 0, "key (D x 2 x key_mod_count x N)"),
                             (out, cols * self._out_limbs(_rescale) * 2, "out (2 x count x L x N)")))
        _require_gpu(scratch)
        if int(count) >= 0 and scratch.numel() * scratch.element_size() < self.scratch_bytes(count, 2):
            raise ValueError("scratch holds fewer than scratch_bytes(count, 2) bytes")
        fn = self._pipeline_fn("multiply_relinearize", _rescale)
        _check(fn(self._h, _ptr(x), _ptr(y), _ptr(key), _ptr(out), int(count), int(bool(output_ntt)), _ptr(scratch),
                  _stream(stream)))

    def relinearize(self, c01, c2, key, out, count, input_ntt, output_ntt, scratch, stream=None):
        """The key switch of `count` three-component ciphertexts: c01 T[2][count][L][N] (any words), c2 T[count][L][N]
        (a contiguous T[3][count][L][N] is c2 = a view of it from word 2 x count x L x N), key the relinearization key,
        out T[2][count][L][N] (may be exactly c01); scratch: at least scratch_bytes(count, 2) bytes, 256-byte aligned.
        out equals apply on c2 plus c01 modulo q, word for word (key_switch.cuh)."""
        if c01 is None or c2 is None or key is None or out is None or scratch is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        self._check_buffers(((c01, cols * self.q_count * 2, "c01 (2 x count x L x N)"),
                             (c2, cols * self.q_count, "c2 (count x L x N)"),
                             (key, self._key_words(2) if cols else 0, "key (D x 2 x key_mod_count x N)"),
                             (out, cols * self.q_count * 2, "out (2 x count x L x N)")))
        _require_gpu(scratch)
        if int(count) >= 0 and scratch.numel() * scratch.element_size() < self.scratch_bytes(count, 2):
            raise ValueError("scratch holds fewer than scratch_bytes(count, 2) bytes")
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_relinearize_u%d" % self.bits)
        _check(fn(self._h, _ptr(c01), _ptr(c2), _ptr(key), _ptr(out), int(count), int(bool(input_ntt)),
                  int(bool(output_ntt)), _ptr(scratch), _stream(stream)))

    def multiply_relinearize_sum(self, xs, ys, key, out, count, output_ntt, scratch, stream=None, _rescale=False):
        """sum_t xs[t] * ys[t] over T = len(xs) pairs of two-component ciphertexts with ONE key switch and ONE ModDown
        (lazy relinearization): xs, ys two lists of T device tensors, 1 <= T <= 32, each T[2][count][L][N] in NTT form
        (any words; ys[t] may be xs[t], a tensor may appear in several terms); key, out, count, output_ntt and scratch as
        for multiply_relinearize; out may be exactly any one of the operands.  With one pair it equals
        multiply_relinearize word for word; it is NOT word for word the sum of T multiply_relinearize results, which
        round T times (key_switch.cuh)."""
        if xs is None or ys is None:
            raise ValueError("null pointer argument")
        xs, ys = list(xs), list(ys)
        if len(xs) != len(ys):
            raise ValueError("multiply_relinearize_sum takes one y per x")
        terms = len(xs)
        if not 1 <= terms <= 32:
            raise ValueError("Invalid terms!")
        if key is None or out is None or scratch is None or any(t is None for t in xs + ys):
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        ct = cols * self.q_count * 2
        self._check_buffers([(t, ct, "x[%d] (2 x count x L x N)" % i) for i, t in enumerate(xs)] +
                            [(t, ct, "y[%d] (2 x count x L x N)" % i) for i, t in enumerate(ys)] +
                            [(key, self._key_words(2) if cols else 0, "key (D x 2 x key_mod_count x N)"),
                             (out, cols * self._out_limbs(_rescale) * 2, "out (2 x count x L x N)")])
        _require_gpu(scratch)
        if int(count) >= 0 and scratch.numel() * scratch.element_size() < self.scratch_bytes(count, 2):
            raise ValueError("scratch holds fewer than scratch_bytes(count, 2) bytes")
        x_ptrs = (ctypes.c_void_p * terms)(*[t.data_ptr() for t in xs])
        y_ptrs = (ctypes.c_void_p * terms)(*[t.data_ptr() for t in ys])
        fn = self._pipeline_fn("multiply_relinearize_sum", _rescale)
        _check(fn(self._h, x_ptrs, y_ptrs, terms, _ptr(key), _ptr(out), int(count), int(bool(output_ntt)),
                  _ptr(scratch), _stream(stream)))

    # ---- rescaling: a plan built with rescale_limbs = R > 0 (key_switch.cuh, "Rescaling"); L' = L - R = kept_count ----
    def _out_limbs(self, rescale):
        """limbs per stack of a pipeline call's out; a *_rescale call on a plan with R = 0 is refused here as the library
        refuses it"""
        if rescale and self._rescale_limbs == 0:
            raise ValueError("The plan was built without rescale_limbs!")
        return self.kept_count if rescale else self.q_count

    def _pipeline_fn(self, name, rescale):
        return getattr(load_library(), "gpuntt_keyswitch_plan_%s%s_u%d" % (name, "_rescale" if rescale else "", self.bits))

    def mod_down_rescale(self, device_x, device_out, stacks, stream=None):
        """device_x T[stacks][M][N] -> device_out T[stacks][L'][N]: divided by P and the R dropped primes with ONE
        rounding; one kernel launch"""
        if device_x is None or device_out is None:
            raise ValueError("null pointer argument")
        cols = self._cols(stacks)
        self._check_buffers(((device_x, cols * self.mod_count, "x (stacks x M x N)"),
                             (device_out, cols * self._out_limbs(True), "out (stacks x L' x N)")))
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_mod_down_rescale_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_x), _ptr(device_out), int(stacks), _stream(stream)))

    def rescale_scratch_bytes(self, stacks):
        """the scratch of rescale(ntt_form=True): T[stacks][R][N], rounded up to 256"""
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_keyswitch_plan_rescale_scratch_bytes_u%d" % self.bits)(
            self._h, int(stacks), ctypes.byref(out)))
        return int(out.value)

    def rescale(self, device_x, device_out, stacks, ntt_form=False, scratch=None, stream=None):
        """device_x T[stacks][L][N] over the q-base (any words) -> device_out T[stacks][L'][N], divided by the R dropped
        primes.  ntt_form False: coefficient form, one kernel launch, no scratch.  ntt_form True: both in NTT form; scratch
        a device tensor of at least rescale_scratch_bytes(stacks) bytes, 256-byte aligned; only the dropped limbs are
        inverse-transformed."""
        if device_x is None or device_out is None:
            raise ValueError("null pointer argument")
        cols = self._cols(stacks)
        self._check_buffers(((device_x, cols * self.q_count, "x (stacks x L x N)"),
                             (device_out, cols * self._out_limbs(True), "out (stacks x L' x N)")))
        if ntt_form:
            _require_gpu(scratch)
            if scratch is None:
                raise ValueError("null pointer argument")
            if int(stacks) >= 0 and scratch.numel() * scratch.element_size() < self.rescale_scratch_bytes(stacks):
                raise ValueError("scratch holds fewer than rescale_scratch_bytes(stacks) bytes")
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_rescale_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_x), _ptr(device_out), int(stacks), int(bool(ntt_form)), _ptr(scratch),
                  _stream(stream)))

    def multiply_relinearize_rescale(self, x, y, key, out, count, output_ntt, scratch, stream=None):
        """multiply_relinearize with the rescale in its ModDown: out T[2][count][L'][N], rounded once (within 1 per
        coefficient of multiply_relinearize followed by rescale, not word for word equal to it)"""
        self.multiply_relinearize(x, y, key, out, count, output_ntt, scratch, stream, _rescale=True)

    def multiply_relinearize_sum_rescale(self, xs, ys, key, out, count, output_ntt, scratch, stream=None):
        """multiply_relinearize_sum with the rescale in its ModDown: out T[2][count][L'][N]"""
        self.multiply_relinearize_sum(xs, ys, key, out, count, output_ntt, scratch, stream, _rescale=True)

    def rotate_hoisted_sum_rescale(self, a, c0, keys, elements, weights, out, count, output_ntt=False, scratch=None,
                                   stream=None):
        """rotate_hoisted_sum with the rescale in its ModDown: out T[2][count][L'][N]"""
        self.rotate_hoisted_sum(a, c0, keys, elements, weights, out, count, output_ntt, scratch, stream, _rescale=True)

    # ---- the double-hoisted baby-step/giant-step linear transform (key_switch.cuh, "linear_transform_bsgs") ----
    def bsgs_scratch_bytes(self, count, n1, n2):
        """the caller-owned scratch of linear_transform_bsgs, in bytes"""
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_keyswitch_plan_bsgs_scratch_bytes_u%d" % self.bits)(
            self.q_count, self.p_count, self.alpha, self.n_power, int(count), int(n1), int(n2), ctypes.byref(out)))
        return int(out.value)

    def linear_transform_bsgs(self, a, c0, c1, baby_keys, baby_elements, giant_keys, giant_elements, weights, out, count,
                              output_ntt=False, scratch=None, stream=None, _rescale=False):
        """out = sum_g sigma_{k_g}(sum_b pt_{g,b} (.) sigma_{k_b}(ct)) with n1 + n2 keys and ONE ModDown: a
        T[D][count][M][N] (what decompose writes), c0 / c1 T[count][L][N] in NTT form (c0 may be None; c1 is needed only
        if a baby key is None), baby_keys / giant_keys lists of n1 / n2 device tensors -- None = no key switch for that
        step, accepted only where the element is 1 -- baby_elements / giant_elements lists of odd ints, weights a list
        of n2 lists of n1 entries, each a device tensor of at least M x N words (the diagonal in NTT form over the full
        base) or None = the term is ABSENT (weight 0; unlike rotate_hoisted_sum, where None means 1); out
        T[2][count][L][N]; scratch: a device tensor of at least bsgs_scratch_bytes(count, n1, n2) bytes, 256-byte
        aligned.  The diagonal is applied BEFORE the giant rotation (key_switch.cuh)."""
        if baby_keys is None or baby_elements is None or giant_keys is None or giant_elements is None or weights is None:
            raise ValueError("null pointer argument")
        baby_keys, giant_keys = list(baby_keys), list(giant_keys)
        baby_elements, giant_elements = [int(k) for k in baby_elements], [int(k) for k in giant_elements]
        n1, n2, cols = len(baby_elements), len(giant_elements), self._cols(count)
        if len(baby_keys) != n1 or len(giant_keys) != n2:
            raise ValueError("linear_transform_bsgs takes one key (or None) per Galois element")
        if not (1 <= n1 <= 64 and 1 <= n2 <= 64 and n1 * n2 <= 256):
            raise ValueError("Invalid baby or giant step count!")
        weights = [None if row is None else list(row) for row in weights]
        if len(weights) != n2 or any(row is None or len(row) != n1 for row in weights):
            raise ValueError("linear_transform_bsgs takes n2 lists of n1 weights (or None)")
        if a is None or out is None or scratch is None:
            raise ValueError("null pointer argument")
        sized = [(a, cols * self.mod_count * self.digits, "a (D x count x M x N)"),
                 (out, cols * self._out_limbs(_rescale) * 2, "out (2 x count x L x N)")]
        sized += [(c, cols * self.q_count, "c%d (count x L x N)" % i) for i, c in enumerate((c0, c1)) if c is not None]
        sized += [(k, self._key_words(2) if cols else 0, "key (D x 2 x key_mod_count x N)")
                  for k in baby_keys + giant_keys if k is not None]
        flat = [w for row in weights for w in row]
        sized += [(w, self.mod_count << self.n_power if cols else 0, "weight (M x N)") for w in flat if w is not None]
        self._check_buffers(sized)
        _require_gpu(scratch)
        if int(count) >= 0 and scratch.numel() * scratch.element_size() < self.bsgs_scratch_bytes(count, n1, n2):
            raise ValueError("scratch holds fewer than bsgs_scratch_bytes(count, n1, n2) bytes")

        def ptrs(ts):
            return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])

        def elts(ks):
            return (ctypes.c_uint32 * len(ks))(*[k & 0xFFFFFFFF for k in ks])

        fn = self._pipeline_fn("linear_transform_bsgs", _rescale)
        _check(fn(self._h, _ptr(a), _ptr(c0), _ptr(c1), ptrs(baby_keys), elts(baby_elements), n1, ptrs(giant_keys),
                  elts(giant_elements), n2, ptrs(flat), _ptr(out), int(count), int(bool(output_ntt)), _ptr(scratch),
                  _stream(stream)))

    def linear_transform_bsgs_rescale(self, a, c0, c1, baby_keys, baby_elements, giant_keys, giant_elements, weights, out,
                                      count, output_ntt=False, scratch=None, stream=None):
        """linear_transform_bsgs with the rescale in its ModDown: out T[2][count][L'][N]"""
        self.linear_transform_bsgs(a, c0, c1, baby_keys, baby_elements, giant_keys, giant_elements, weights, out, count,
                                   output_ntt, scratch, stream, _rescale=True)

    # key material (key_switch.cuh, "Key material")
    @staticmethod
    def _check_small(t, words, name):
        _require_gpu(t)
        if t.element_size() != 4 or t.dtype.is_floating_point:
            raise ValueError("%s takes 32-bit signed integer tensors" % name)
        if words > 0 and t.numel() < words:
            raise ValueError("%s needs %d words; got %d" % (name, words, t.numel()))

    def _check_aligned_scratch(self, scratch, need, name):
        _require_gpu(scratch)
        if scratch.numel() * scratch.element_size() < need:
            raise ValueError("scratch holds fewer than %s bytes" % name)

    def lift_small(self, small, out, polys, full_base=True, to_ntt=True, stream=None):
        """small int32[polys][N] (any values) -> out T[polys][M or L][N]: the canonical residue of every signed value under
        every modulus of the full base (full_base) or the q-base; with to_ntt the plan's forward transform over that base
        follows in place.  One launch plus the transform's own."""
        if small is None or out is None:
            raise ValueError("null pointer argument")
        cols = self._cols(polys)
        self._check_small(small, cols, "small (polys x N)")
        self._check_buffers(((out, cols * (self.mod_count if full_base else self.q_count), "out (polys x B x N)"),))
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_lift_small_u%d" % self.bits)
        _check(fn(self._h, _ptr(small), _ptr(out), int(polys), int(bool(full_base)), int(bool(to_ntt)),
                  _stream(stream)))

    def keygen_scratch_bytes(self, keys):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_keyswitch_plan_keygen_scratch_bytes_u%d" % self.bits)(
            self._h, int(keys), ctypes.byref(out)))
        return int(out.value)

    def encrypt_scratch_bytes(self, count):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_keyswitch_plan_encrypt_scratch_bytes_u%d" % self.bits)(
            self._h, int(count), ctypes.byref(out)))
        return int(out.value)

    def generate_keys(self, s, s_from, errors, keys, scratch, stream=None):
        """len(keys) <= 64 switching keys to the secret s in one call: s T[M][N] and s_from T[len(keys)][M][N] in NTT form
        over the full base (lift_small gives them), errors int32[len(keys)][D][N], keys a list of device tensors, each
        T[D][2][M][N] with component 1 = a on entry (sample_uniform fills it in place); component 0 =
        E - a s + P g_d s_from is written, a is left untouched.  scratch: at least keygen_scratch_bytes(len(keys)) bytes,
        256-byte aligned.  Word for word the header's definition (key_switch.cuh)."""
        keys = list(keys)
        G = len(keys)
        if not 0 <= G <= 64:
            raise ValueError("Invalid keys!")
        if s is None or s_from is None or errors is None or scratch is None or any(k is None for k in keys):
            raise ValueError("null pointer argument")
        stack = self.mod_count << self.n_power
        self._check_buffers([(s, stack, "s (M x N)"), (s_from, stack * G, "s_from (keys x M x N)")] +
                            [(k, 2 * self.digits * stack, "key (D x 2 x M x N)") for k in keys])
        self._check_small(errors, (G * self.digits) << self.n_power, "errors (keys x D x N)")
        self._check_aligned_scratch(scratch, self.keygen_scratch_bytes(G), "keygen_scratch_bytes(keys)")
        key_ptrs = (ctypes.c_void_p * max(1, G))(*[k.data_ptr() for k in keys])
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_generate_keys_u%d" % self.bits)
        _check(fn(self._h, _ptr(s), _ptr(s_from), _ptr(errors), key_ptrs, G, _ptr(scratch), _stream(stream)))

    def encrypt_symmetric(self, s, errors, message, out, count, scratch, stream=None):
        """`count` symmetric encryptions under s T[M][N] (NTT form; the first L limbs are read): out T[2][count][L][N] with
        out[1] = a on entry (left untouched), errors int32[count][N], message T[count][L][N] in NTT form or None (an
        encryption of zero: a public key); out[0] = E - a s + message is written.  scratch: at least
        encrypt_scratch_bytes(count) bytes, 256-byte aligned."""
        if s is None or errors is None or out is None or scratch is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        sized = [(s, self.q_count << self.n_power, "s (L x N at least)"),
                 (out, 2 * cols * self.q_count, "out (2 x count x L x N)")]
        if message is not None:
            sized.append((message, cols * self.q_count, "message (count x L x N)"))
        self._check_buffers(sized)
        self._check_small(errors, cols, "errors (count x N)")
        if int(count) >= 0:
            self._check_aligned_scratch(scratch, self.encrypt_scratch_bytes(count), "encrypt_scratch_bytes(count)")
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_encrypt_symmetric_u%d" % self.bits)
        _check(fn(self._h, _ptr(s), _ptr(errors), _ptr(message), _ptr(out), int(count), _ptr(scratch),
                  _stream(stream)))

    # decryption and public-key encryption (key_switch.cuh, "Decryption and public-key encryption")
    def phase_scratch_bytes(self, count, components=2, input_ntt=True):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_keyswitch_plan_phase_scratch_bytes_u%d" % self.bits)(
            self._h, int(count), int(components), int(bool(input_ntt)), ctypes.byref(out)))
        return int(out.value)

    def phase(self, ct, s, out, count, components=2, input_ntt=True, output_ntt=False, scratch=None, stream=None):
        """c0 + c1 s [+ c2 s^2]: ct T[components][count][L][N] (components 2 or 3), s T[M][N] in NTT form (the first L
        limbs are read) -> out T[count][L][N]; out may be ct itself in NTT form.  scratch: at least
        phase_scratch_bytes(count, components, input_ntt) bytes, 256-byte aligned (None for NTT-form input)."""
        if ct is None or s is None or out is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        comps = int(components) if int(components) in (2, 3) else 0
        self._check_buffers([(ct, comps * cols * self.q_count, "ct (components x count x L x N)"),
                             (s, self.q_count << self.n_power, "s (L x N at least)"),
                             (out, cols * self.q_count, "out (count x L x N)")])
        if scratch is not None and comps and int(count) >= 0:
            self._check_aligned_scratch(scratch, self.phase_scratch_bytes(count, components, input_ntt),
                                        "phase_scratch_bytes(count, components, input_ntt)")
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_phase_u%d" % self.bits)
        _check(fn(self._h, _ptr(ct), _ptr(s), _ptr(out), int(count), int(components), int(bool(input_ntt)),
                  int(bool(output_ntt)), _ptr(scratch), _stream(stream)))

    def encrypt_public_scratch_bytes(self, count):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_keyswitch_plan_encrypt_public_scratch_bytes_u%d" % self.bits)(
            self._h, int(count), ctypes.byref(out)))
        return int(out.value)

    def encrypt_public(self, pk, small, message, out, count, scratch, stream=None):
        """`count` public-key encryptions: pk T[2][L][N] in NTT form (what encrypt_symmetric(count=1, message=None)
        leaves in out), small int32[3][count][N] = (u, e0, e1), message T[count][L][N] in NTT form or None ->
        out T[2][count][L][N] = (pk0 U + E0 + message, pk1 U + E1).  scratch: at least
        encrypt_public_scratch_bytes(count) bytes, 256-byte aligned."""
        if pk is None or small is None or out is None or scratch is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        sized = [(pk, (2 * self.q_count) << self.n_power, "pk (2 x L x N)"),
                 (out, 2 * cols * self.q_count, "out (2 x count x L x N)")]
        if message is not None:
            sized.append((message, cols * self.q_count, "message (count x L x N)"))
        self._check_buffers(sized)
        self._check_small(small, 3 * cols, "small (3 x count x N)")
        if int(count) >= 0:
            self._check_aligned_scratch(scratch, self.encrypt_public_scratch_bytes(count),
                                        "encrypt_public_scratch_bytes(count)")
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_encrypt_public_u%d" % self.bits)
        _check(fn(self._h, _ptr(pk), _ptr(small), _ptr(message), _ptr(out), int(count), _ptr(scratch),
                  _stream(stream)))

    # plaintext operands (key_switch.cuh, "Plaintext operands")
    def lift_centred(self, words, plain_modulus, out, polys, full_base=True, to_ntt=True, stream=None):
        """words T[polys][N] (any words, read modulo plain_modulus and centred: m - t from (t + 1) >> 1 on) -> out
        T[polys][M or L][N], the canonical residues; with to_ntt the plan's forward transform over that base follows in
        place.  One launch plus the transform's own.  How a plaintext (BfvBatchEncoder.encode) becomes an operand of
        multiply_plain (q-base) or a diagonal of rotate_hoisted_sum / linear_transform_bsgs (full base)."""
        if words is None or out is None:
            raise ValueError("null pointer argument")
        if not 0 <= int(plain_modulus) < 1 << self.bits:
            raise ValueError("Invalid plaintext modulus!")
        cols = self._cols(polys)
        self._check_buffers(((words, cols, "words (polys x N)"),
                             (out, cols * (self.mod_count if full_base else self.q_count), "out (polys x B x N)")))
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_lift_centred_u%d" % self.bits)
        _check(fn(self._h, _ptr(words), _ct(self.bits)(int(plain_modulus)), _ptr(out), int(polys),
                  int(bool(full_base)), int(bool(to_ntt)), _stream(stream)))

    def multiply_plain(self, ct, pt, out, count, plain_count=1, stream=None):
        """ct T[2][count][L][N] times pt T[plain_count][L][N] word by word modulo q_i, both in NTT form and any words;
        plain_count 1 (one plaintext for every ciphertext) or count -> out T[2][count][L][N], canonical; out may be ct
        itself.  One launch."""
        if ct is None or pt is None or out is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        pc = int(plain_count) if int(plain_count) in (1, int(count)) else 0
        self._check_buffers(((ct, 2 * cols * self.q_count, "ct (2 x count x L x N)"),
                             (pt, (pc * self.q_count) << self.n_power, "pt (plain_count x L x N)"),
                             (out, 2 * cols * self.q_count, "out (2 x count x L x N)")))
        fn = getattr(load_library(), "gpuntt_keyswitch_plan_multiply_plain_u%d" % self.bits)
        _check(fn(self._h, _ptr(ct), _ptr(pt), _ptr(out), int(count), int(plain_count), _stream(stream)))

    def close(self):
        if self._h:
            getattr(load_library(), "gpuntt_keyswitch_plan_destroy_u%d" % self.bits)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------- samplers (rns/sampling.cuh)
TERNARY, CBD21 = 0, 1
SAMPLE_MAX_CANDIDATES = 32


def philox4x32_10(ctr, key):
    """Host (no GPU): the standard Philox4x32-10 block of the 4 counter words and 2 key words, as 4 ints"""
    c = (ctypes.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in ctr])
    k = (ctypes.c_uint32 * 2)(*[int(v) & 0xFFFFFFFF for v in key])
    out = (ctypes.c_uint32 * 4)()
    _check(load_library().gpuntt_philox4x32_10(c, k, out))
    return [int(v) for v in out]


def _sample_args(moduli, n_power, stacks, stack_stride_words, bits):
    vals = [int(getattr(m, "value", m)) for m in moduli]
    if not 1 <= len(vals) <= 256:
        raise ValueError("Invalid mod_count!")
    if any(not 0 < v < (1 << bits) for v in vals):
        raise ValueError("Invalid modulus!")
    dense = len(vals) << int(n_power)
    stride = dense if stack_stride_words is None else int(stack_stride_words)
    if stride < dense:
        raise ValueError("Invalid stack stride!")
    words = (int(stacks) - 1) * stride + dense if int(stacks) > 0 else 0
    return (_ct(bits) * len(vals))(*vals), len(vals), stride, words


def sample_uniform(out, moduli, n_power, stacks, seed, stream_id=0, stack_stride_words=None, stream=None):
    """Fill out T[stacks][len(moduli)][N] (stack s at s x stack_stride_words, default dense) with uniform residues:
    a pure function of (seed, stream_id, word index), restated in tests/sampling_exact.py.  NOT a cryptographic
    generator (sampling.cuh).  One launch; 16-byte stores where out and the stride allow."""
    if out is None:
        raise ValueError("null pointer argument")
    _require_gpu(out)
    bits = out.element_size() * 8
    if bits not in (32, 64) or out.dtype.is_floating_point:
        raise ValueError("sample_uniform fills 32- or 64-bit integer tensors")
    arr, count, stride, words = _sample_args(moduli, n_power, stacks, stack_stride_words, bits)
    if out.numel() < words:
        raise ValueError("out needs %d words; got %d" % (words, out.numel()))
    fn = getattr(load_library(), "gpuntt_sample_uniform_u%d" % bits)
    _check(fn(_ptr(out), arr, count, int(n_power), int(stacks), ctypes.c_uint64(stride),
              ctypes.c_uint64(int(seed) & (2**64 - 1)), ctypes.c_uint32(int(stream_id) & 0xFFFFFFFF), _stream(stream)))


def sample_small(out, polys, n_power, distribution, seed, stream_id=0, stream=None):
    """Fill out int32[polys][N] with TERNARY (uniform on -1, 0, 1) or CBD21 (centred binomial, variance 10.5) values, a
    pure function of (seed, stream_id, word index).  One launch."""
    if out is None:
        raise ValueError("null pointer argument")
    _require_gpu(out)
    if out.element_size() != 4 or out.dtype.is_floating_point:
        raise ValueError("sample_small fills 32-bit signed integer tensors")
    if int(polys) > 0 and out.numel() < int(polys) << int(n_power):
        raise ValueError("out needs %d words; got %d" % (int(polys) << int(n_power), out.numel()))
    _check(load_library().gpuntt_sample_small(
        _ptr(out), int(polys), int(n_power), int(distribution), ctypes.c_uint64(int(seed) & (2**64 - 1)),
        ctypes.c_uint32(int(stream_id) & 0xFFFFFFFF), _stream(stream)))


def sample_reference_uniform(moduli, n_power, stacks, seed, stream_id=0, stack_stride_words=None, bits=64,
                             max_candidates=SAMPLE_MAX_CANDIDATES, fill=0):
    """Host (no GPU): sample_uniform's words as a numpy array of (stacks - 1) x stride + len(moduli) x N words, the gaps
    between strided stacks left at `fill`; max_candidates < 32 reaches the `r mod q` tail"""
    arr, count, stride, words = _sample_args(moduli, n_power, stacks, stack_stride_words, bits)
    out = np.full(max(1, words), fill, dtype=np_dtype(bits))
    fn = getattr(load_library(), "gpuntt_sample_reference_uniform_u%d" % bits)
    _check(fn(out.ctypes.data_as(ctypes.c_void_p), arr, count, int(n_power), int(stacks), ctypes.c_uint64(stride),
              ctypes.c_uint64(int(seed) & (2**64 - 1)), ctypes.c_uint32(int(stream_id) & 0xFFFFFFFF),
              int(max_candidates)))
    return out[:words]


def sample_reference_small(polys, n_power, distribution, seed, stream_id=0):
    """Host (no GPU): sample_small's words as a numpy int32 array of polys x N"""
    words = int(polys) << int(n_power) if int(polys) > 0 else 0
    out = np.zeros(max(1, words), dtype=np.int32)
    _check(load_library().gpuntt_sample_reference_small(
        out.ctypes.data_as(ctypes.c_void_p), int(polys), int(n_power), int(distribution),
        ctypes.c_uint64(int(seed) & (2**64 - 1)), ctypes.c_uint32(int(stream_id) & 0xFFFFFFFF)))
    return out[:words]


def bfv_constants(q_moduli, b_moduli, plain_modulus, n_power, bits=64):
    """Host (no GPU): the constants a BfvMultiplyPlan of these bases and this t uploads (BfvConstants<T>), as a dict of
    numpy arrays -- up_* the seven arrays of baseconv_constants({q} -> {b}), down_* those of {b} -> {q}, t_mod[M],
    t_mod_shoup[M], t_qhat_inv[L] ((t qhat_i^-1) mod q_i) and t_qhat_inv_shoup[L].  Raises ValueError where the plan's
    constructor would ("Auxiliary base too small!" among them)."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    bs, barr = _keyswitch_moduli(b_moduli, bits)
    L, K, dt = len(qs), len(bs), np_dtype(bits)
    side = lambda a, b: (("qhat_inv", (a,)), ("qhat_inv_shoup", (a,)), ("matrix", (a, b)), ("q_mod_p", (b,)),
                         ("q_inv_mod_p", (b,)), ("recip", (a,)), ("bit_length", (a,)))
    shapes = tuple(("up_" + n, s) for n, s in side(L, K)) + tuple(("down_" + n, s) for n, s in side(K, L)) + \
        (("t_mod", (L + K,)), ("t_mod_shoup", (L + K,)), ("t_qhat_inv", (L,)), ("t_qhat_inv_shoup", (L,)))
    out = {name: np.zeros(tuple(max(1, d) for d in shape), dtype=dt) for name, shape in shapes}
    ptrs = (ctypes.c_void_p * len(shapes))(*[out[name].ctypes.data for name, _ in shapes])
    fn = getattr(load_library(), "gpuntt_bfv_constants_u%d" % bits)
    _check(fn(qarr, L, barr, K, _ct(bits)(int(plain_modulus) & ((1 << bits) - 1)), int(n_power), ptrs))
    return out


def bfv_max_terms(q_moduli, b_moduli, plain_modulus, n_power, bits=64):
    """Host (no GPU): BfvMultiplyPlan<T>::max_terms of a plan of these bases, this t and this ring --
    min(32, B // (2 t N Q)) -- with the checks of the constructor ("Auxiliary base too small!" where that is 0)."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    bs, barr = _keyswitch_moduli(b_moduli, bits)
    out = ctypes.c_int()
    fn = getattr(load_library(), "gpuntt_bfv_max_terms_u%d" % bits)
    _check(fn(qarr, len(qs), barr, len(bs), _ct(bits)(int(plain_modulus) & ((1 << bits) - 1)), int(n_power),
              ctypes.byref(out)))
    return int(out.value)


def bfv_reference_extend(q_moduli, b_moduli, x, full, n_power, stacks, bits=64):
    """Host (no GPU): BfvMultiplyPlan<T>::reference_extend on numpy arrays of the plan's word type -- x holds stacks x L
    x N words, full stacks x M x N (written and returned) -- after the argument checks of extend (ValueError).  None for
    an array is the C NULL."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    bs, barr = _keyswitch_moduli(b_moduli, bits)
    L, M = len(qs), len(qs) + len(bs)
    ok = 1 <= int(n_power) <= 28 and int(stacks) >= 0
    cols = (int(stacks) << int(n_power)) if ok else None
    px = _keyswitch_host_array(x, bits, cols * L if ok else None, "in (stacks x L x N)")
    pf = _keyswitch_host_array(full, bits, cols * M if ok else None, "full (stacks x M x N)")
    fn = getattr(load_library(), "gpuntt_bfv_reference_extend_u%d" % bits)
    _check(fn(qarr, len(qs), barr, len(bs), px, pf, int(n_power), int(stacks)))
    return full


def bfv_reference_scale_round(q_moduli, b_moduli, plain_modulus, full, out, n_power, stacks, bits=64):
    """Host (no GPU): BfvMultiplyPlan<T>::reference_scale_round -- full holds stacks x M x N words, out stacks x L x N
    (written and returned)."""
    qs, qarr = _keyswitch_moduli(q_moduli, bits)
    bs, barr = _keyswitch_moduli(b_moduli, bits)
    L, M = len(qs), len(qs) + len(bs)
    ok = 1 <= int(n_power) <= 28 and int(stacks) >= 0
    cols = (int(stacks) << int(n_power)) if ok else None
    pf = _keyswitch_host_array(full, bits, cols * M if ok else None, "full (stacks x M x N)")
    po = _keyswitch_host_array(out, bits, cols * L if ok else None, "out (stacks x L x N)")
    fn = getattr(load_library(), "gpuntt_bfv_reference_scale_round_u%d" % bits)
    _check(fn(qarr, len(qs), barr, len(bs), _ct(bits)(int(plain_modulus) & ((1 << bits) - 1)), pf, po, int(n_power),
              int(stacks)))
    return out


def noise_budget_bits(noise_max, q_count, bits=64):
    """Host (no GPU): SEAL's invariant noise budget in bits from BfvMultiplyPlan.decode's noise_max over q_count limbs,
    max(0, W - 1 - bit_length(noise_max + 3 q_count)) -- conservative by decode's band (bfv_multiply.cuh)"""
    return max(0, int(bits) - 1 - (int(noise_max) + 3 * int(q_count)).bit_length())


class BfvMultiplyPlan:
    """Extension BfvMultiplyPlan<T> (include/gpuntt/rns/bfv_multiply.cuh): the scale-invariant product
    round(t (x (x) y) / Q) for the q-base `q_moduli` (L), the auxiliary base `b_moduli` (K, B >= 2 t N Q or ValueError
    "Auxiliary base too small!") and the plaintext modulus `plain_modulus` on a ring of 2^n_power, M = L + K <= 64.
    forward_table / inverse_table: device tensors as for GPU_NTT / GPU_INTT over the full base (slot i at i << n_power),
    mod_inverse the M host n^-1 values; all three None: a plan without transforms (extend / scale_round only).
    `workspace`: an optional uint8 device tensor of workspace_bytes() bytes owned by the caller.  `scratch` of multiply:
    a device tensor of at least plan.scratch_bytes(count) bytes, 256-byte aligned, owned by the caller; nothing is
    allocated by any call."""

    def __init__(self, q_moduli, b_moduli, plain_modulus, n_power, forward_table=None, inverse_table=None,
                 mod_inverse=None, reduction_poly=X_N_plus, batch_hint=1024, bits=64, stream=None, workspace=None):
        lib = load_library()
        qs, qarr = _keyswitch_moduli(q_moduli, bits)
        bs, barr = _keyswitch_moduli(b_moduli, bits)
        _require_gpu(workspace, forward_table, inverse_table)
        self.bits, self.q_count, self.b_count, self.mod_count = bits, len(qs), len(bs), len(qs) + len(bs)
        self.n_power, self.plain_modulus = int(n_power), int(plain_modulus)
        for t in (forward_table, inverse_table):
            if t is not None and (t.element_size() * 8 != bits or t.numel() < self.mod_count << self.n_power):
                raise ValueError("a table holds M x N %d-bit words" % bits)
        ninv = None
        if mod_inverse is not None:
            vals = [int(v) for v in mod_inverse]
            if len(vals) != self.mod_count:
                raise ValueError("mod_inverse holds one n^-1 per modulus of the full base")
            ninv = (_ct(bits) * max(1, len(vals)))(*vals)
        if workspace is not None:
            need = self.workspace_bytes(len(qs), len(bs), n_power, bits)  # raises for counts out of range
            if workspace.numel() * workspace.element_size() < need:
                raise ValueError("workspace holds fewer than workspace_bytes() bytes")
        self._keep = (workspace, forward_table, inverse_table)
        self._h = ctypes.c_void_p()
        fn = getattr(lib, "gpuntt_bfv_plan_create_u%d" % bits)
        _check(fn(ctypes.byref(self._h), qarr, len(qs), barr, len(bs),
                  _ct(bits)(self.plain_modulus & ((1 << bits) - 1)), int(n_power), _ptr(forward_table),
                  _ptr(inverse_table), ninv, int(reduction_poly), int(batch_hint), _ptr(workspace), _stream(stream)))

    @staticmethod
    def workspace_bytes(q_count, b_count, n_power, bits=64):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_bfv_plan_workspace_bytes_u%d" % bits)(
            int(q_count), int(b_count), int(n_power), ctypes.byref(out)))
        return int(out.value)

    def scratch_bytes(self, count):
        """BfvMultiplyPlan<T>::scratch_bytes: the caller-owned scratch of multiply, in bytes"""
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_bfv_plan_scratch_bytes_u%d" % self.bits)(
            self.q_count, self.b_count, self.n_power, int(count), ctypes.byref(out)))
        return int(out.value)

    @property
    def owns_workspace(self):
        """False: the plan lives in the caller's workspace and has allocated no device memory"""
        return bool(getattr(load_library(), "gpuntt_bfv_plan_owns_workspace_u%d" % self.bits)(self._h))

    def _check_buffers(self, sized):
        """the library cannot see tensor sizes or types: sized = (tensor, words needed, name) ...; None is the C NULL,
        which the library refuses"""
        _require_gpu(*[t for t, _, _ in sized])
        for t, words, name in sized:
            if t is None:
                continue
            if t.element_size() * 8 != self.bits or t.dtype.is_floating_point:
                raise ValueError("a %d-bit BfvMultiplyPlan takes %d-bit integer tensors" % (self.bits, self.bits))
            if words > 0 and t.numel() < words:
                raise ValueError("%s needs %d words; got %d" % (name, words, t.numel()))

    def _cols(self, count):
        return (int(count) << self.n_power) if int(count) > 0 else 0

    def extend(self, device_in, device_full, stacks, stream=None):
        """device_in T[stacks][L][N] -> device_full T[stacks][M][N]; one kernel launch"""
        cols = self._cols(stacks)
        self._check_buffers(((device_in, cols * self.q_count, "in (stacks x L x N)"),
                             (device_full, cols * self.mod_count, "full (stacks x M x N)")))
        fn = getattr(load_library(), "gpuntt_bfv_plan_extend_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_in), _ptr(device_full), int(stacks), _stream(stream)))

    def scale_round(self, device_full, device_out, stacks, stream=None):
        """device_full T[stacks][M][N] -> device_out T[stacks][L][N]; one kernel launch"""
        cols = self._cols(stacks)
        self._check_buffers(((device_full, cols * self.mod_count, "full (stacks x M x N)"),
                             (device_out, cols * self.q_count, "out (stacks x L x N)")))
        fn = getattr(load_library(), "gpuntt_bfv_plan_scale_round_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_full), _ptr(device_out), int(stacks), _stream(stream)))

    def multiply(self, x, y, out, count, input_ntt=False, output_ntt=False, scratch=None, stream=None):
        """x, y T[2][count][L][N] (y may be x) -> out T[3][count][L][N]; out may be x or y itself.  scratch: at least
        scratch_bytes(count) bytes, 256-byte aligned"""
        cols = self._cols(count)
        self._check_buffers(((x, cols * self.q_count * 2, "x (2 x count x L x N)"),
                             (y, cols * self.q_count * 2, "y (2 x count x L x N)"),
                             (out, cols * self.q_count * 3, "out (3 x count x L x N)")))
        _require_gpu(scratch)
        if scratch is not None and int(count) > 0 and \
                scratch.numel() * scratch.element_size() < self.scratch_bytes(count):
            raise ValueError("scratch holds fewer than scratch_bytes(count) bytes")
        fn = getattr(load_library(), "gpuntt_bfv_plan_multiply_u%d" % self.bits)
        _check(fn(self._h, _ptr(x), _ptr(y), _ptr(out), int(count), int(bool(input_ntt)), int(bool(output_ntt)),
                  _ptr(scratch), _stream(stream)))

    def multiply_relinearize(self, x, y, key_switch, key, out, count, input_ntt=False, output_ntt=False, scratch=None,
                             key_switch_scratch=None, stream=None):
        """BFV ct x ct in one call: x, y T[2][count][L][N] (y may be x) -> out T[2][count][L][N], the product
        relinearized by the KeySwitchPlan `key_switch` (the same q-base, ring and reduction polynomial, or ValueError
        "The key-switching plan does not match!") under `key`; out may be x or y itself.  scratch: at least
        scratch_bytes(count) bytes; key_switch_scratch: at least key_switch.scratch_bytes(count, 2) bytes; both 256-byte
        aligned.  out equals multiply(output_ntt=False) then key_switch.relinearize word for word (bfv_multiply.cuh)."""
        if not isinstance(key_switch, KeySwitchPlan) or key_switch.bits != self.bits:
            raise ValueError("key_switch is a KeySwitchPlan of the same word width")
        cols = self._cols(count)
        self._check_buffers(((x, cols * self.q_count * 2, "x (2 x count x L x N)"),
                             (y, cols * self.q_count * 2, "y (2 x count x L x N)"),
                             (key, key_switch._key_words(2) if cols else 0, "key (D x 2 x key_mod_count x N)"),
                             (out, cols * self.q_count * 2, "out (2 x count x L x N)")))
        _require_gpu(scratch, key_switch_scratch)
        if scratch is not None and int(count) > 0 and \
                scratch.numel() * scratch.element_size() < self.scratch_bytes(count):
            raise ValueError("scratch holds fewer than scratch_bytes(count) bytes")
        if key_switch_scratch is not None and int(count) > 0 and \
                key_switch_scratch.numel() * key_switch_scratch.element_size() < key_switch.scratch_bytes(count, 2):
            raise ValueError("key_switch_scratch holds fewer than key_switch.scratch_bytes(count, 2) bytes")
        fn = getattr(load_library(), "gpuntt_bfv_plan_multiply_relinearize_u%d" % self.bits)
        _check(fn(self._h, _ptr(x), _ptr(y), key_switch._h, _ptr(key), _ptr(out), int(count), int(bool(input_ntt)),
                  int(bool(output_ntt)), _ptr(scratch), _ptr(key_switch_scratch), _stream(stream)))

    # ---- encode, decode, decrypt (bfv_multiply.cuh, "Reading a result back") ----
    def scale_message(self, message, out, count, to_ntt=True, stream=None):
        """message T[count][N] (any word, read modulo t) -> out T[count][L][N] = round(Q m / t) in the q-base, what
        encrypt_symmetric / encrypt_public take as message; with to_ntt the q-base transform follows in place"""
        if message is None or out is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        self._check_buffers(((message, cols, "message (count x N)"),
                             (out, cols * self.q_count, "out (count x L x N)")))
        fn = getattr(load_library(), "gpuntt_bfv_plan_scale_message_u%d" % self.bits)
        _check(fn(self._h, _ptr(message), _ptr(out), int(count), int(bool(to_ntt)), _stream(stream)))

    def decode_partials_bytes(self, stacks):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_bfv_plan_decode_partials_bytes_u%d" % self.bits)(
            self._h, int(stacks), ctypes.byref(out)))
        return int(out.value)

    def decode(self, x, message_out, noise_max, stacks, stream=None, partials=None):
        """x T[stacks][L][N] in coefficient form (any word) -> message_out T[stacks][N] = round(t x / Q) mod t and, unless
        None, noise_max T[stacks] = the largest |noise word| of every stack (noise_budget_bits turns it into bits).
        partials: None (a memset and one launch) or a device tensor of at least decode_partials_bytes(stacks) bytes --
        the same words from two launches and no memset"""
        if x is None or message_out is None:
            raise ValueError("null pointer argument")
        cols = self._cols(stacks)
        self._check_buffers(((x, cols * self.q_count, "x (stacks x L x N)"), (message_out, cols, "message_out (stacks x N)"),
                             (noise_max, max(0, int(stacks)), "noise_max (stacks)")))
        if partials is not None:
            _require_gpu(partials)
            if int(stacks) > 0 and partials.numel() * partials.element_size() < self.decode_partials_bytes(stacks):
                raise ValueError("partials holds fewer than decode_partials_bytes(stacks) bytes")
            fn = getattr(load_library(), "gpuntt_bfv_plan_decode_two_launch_u%d" % self.bits)
            _check(fn(self._h, _ptr(x), _ptr(message_out), _ptr(noise_max), int(stacks), _ptr(partials), _stream(stream)))
            return
        fn = getattr(load_library(), "gpuntt_bfv_plan_decode_u%d" % self.bits)
        _check(fn(self._h, _ptr(x), _ptr(message_out), _ptr(noise_max), int(stacks), _stream(stream)))

    def decrypt_scratch_bytes(self, count):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_bfv_plan_decrypt_scratch_bytes_u%d" % self.bits)(
            self._h, int(count), ctypes.byref(out)))
        return int(out.value)

    def decrypt(self, ct, key_switch, s, message_out, noise_max, count, components=2, input_ntt=True, scratch=None,
                key_switch_scratch=None, stream=None):
        """key_switch.phase(ct, s, scratch, output_ntt=False) then decode(scratch, message_out, noise_max), word for word:
        ct T[components][count][L][N], s T[M][N] in NTT form -> message_out T[count][N], noise_max T[count] or None.
        scratch: at least decrypt_scratch_bytes(count) bytes; key_switch_scratch: at least
        key_switch.phase_scratch_bytes(count, components, input_ntt) bytes (None where that is 0); 256-byte aligned."""
        if not isinstance(key_switch, KeySwitchPlan) or key_switch.bits != self.bits:
            raise ValueError("key_switch is a KeySwitchPlan of the same word width")
        if ct is None or s is None or message_out is None or scratch is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        comps = int(components) if int(components) in (2, 3) else 0
        self._check_buffers(((ct, comps * cols * self.q_count, "ct (components x count x L x N)"),
                             (s, self.q_count << self.n_power, "s (L x N at least)"),
                             (message_out, cols, "message_out (count x N)"),
                             (noise_max, max(0, int(count)), "noise_max (count)")))
        _require_gpu(scratch, key_switch_scratch)
        if int(count) > 0 and scratch.numel() * scratch.element_size() < self.decrypt_scratch_bytes(count):
            raise ValueError("scratch holds fewer than decrypt_scratch_bytes(count) bytes")
        if key_switch_scratch is not None and int(count) > 0 and comps and \
                key_switch_scratch.numel() * key_switch_scratch.element_size() < \
                key_switch.phase_scratch_bytes(count, components, input_ntt):
            raise ValueError("key_switch_scratch holds fewer than key_switch.phase_scratch_bytes(...) bytes")
        fn = getattr(load_library(), "gpuntt_bfv_plan_decrypt_u%d" % self.bits)
        _check(fn(self._h, _ptr(ct), key_switch._h, _ptr(s), _ptr(message_out), _ptr(noise_max), int(count),
                  int(components), int(bool(input_ntt)), _ptr(scratch), _ptr(key_switch_scratch), _stream(stream)))

    # ---- the summed product (bfv_multiply.cuh, "multiply_sum") ----
    @property
    def max_terms(self):
        """BfvMultiplyPlan<T>::max_terms: min(32, B // (2 t N Q)), the most terms one multiply_sum call may add up"""
        rc = getattr(load_library(), "gpuntt_bfv_plan_max_terms_u%d" % self.bits)(self._h)
        if rc < 0:
            _check(rc)
        return int(rc)

    def sum_scratch_bytes(self, count, operands):
        """BfvMultiplyPlan<T>::sum_scratch_bytes: the scratch of multiply_sum for `operands` distinct operand tensors"""
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_bfv_plan_sum_scratch_bytes_u%d" % self.bits)(
            self.q_count, self.b_count, self.n_power, int(count), int(operands), ctypes.byref(out)))
        return int(out.value)

    def _sum_operands(self, xs, ys, out, comps, count, scratch):
        """the checks multiply_sum and multiply_relinearize_sum share; returns (terms, x pointers, y pointers)"""
        if xs is None or ys is None:
            raise ValueError("null pointer argument")
        xs, ys = list(xs), list(ys)
        if len(xs) != len(ys):
            raise ValueError("multiply_sum takes one y per x")
        terms = len(xs)
        if not 1 <= terms <= 32:
            raise ValueError("Invalid terms!")
        if out is None or scratch is None or any(t is None for t in xs + ys):
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        ct = cols * self.q_count * 2
        self._check_buffers([(t, ct, "x[%d] (2 x count x L x N)" % i) for i, t in enumerate(xs)] +
                            [(t, ct, "y[%d] (2 x count x L x N)" % i) for i, t in enumerate(ys)] +
                            [(out, cols * self.q_count * comps, "out (%d x count x L x N)" % comps)])
        _require_gpu(scratch)
        distinct = len({t.data_ptr() for t in xs + ys})
        if int(count) > 0 and scratch.numel() * scratch.element_size() < self.sum_scratch_bytes(count, distinct):
            raise ValueError("scratch holds fewer than sum_scratch_bytes(count, %d) bytes: the call has %d distinct "
                             "operands" % (distinct, distinct))
        x_ptrs = (ctypes.c_void_p * terms)(*[t.data_ptr() for t in xs])
        y_ptrs = (ctypes.c_void_p * terms)(*[t.data_ptr() for t in ys])
        return terms, x_ptrs, y_ptrs

    def multiply_sum(self, xs, ys, out, count, input_ntt=False, output_ntt=False, scratch=None, stream=None):
        """sum_t xs[t] * ys[t] with ONE division by Q: xs, ys two lists of T device tensors, 1 <= T <= max_terms, each
        T[2][count][L][N] with multiply's rules (ys[t] may be xs[t]; a tensor may appear in several terms and is extended
        and transformed once) -> out T[3][count][L][N]; out may be exactly one operand.  scratch: at least
        sum_scratch_bytes(count, U) bytes for the U distinct tensors, 256-byte aligned.  With one pair it equals multiply
        word for word; with more it rounds once where T multiply calls round T times (bfv_multiply.cuh)."""
        terms, x_ptrs, y_ptrs = self._sum_operands(xs, ys, out, 3, count, scratch)
        fn = getattr(load_library(), "gpuntt_bfv_plan_multiply_sum_u%d" % self.bits)
        _check(fn(self._h, x_ptrs, y_ptrs, terms, _ptr(out), int(count), int(bool(input_ntt)), int(bool(output_ntt)),
                  _ptr(scratch), _stream(stream)))

    def multiply_relinearize_sum(self, xs, ys, key_switch, key, out, count, input_ntt=False, output_ntt=False,
                                 scratch=None, key_switch_scratch=None, stream=None):
        """An encrypted BFV dot product in one call: multiply_sum(output_ntt=False), then key_switch.relinearize -> out
        T[2][count][L][N], with ONE t/Q rounding, ONE key switch and ONE ModDown.  xs, ys, scratch as for multiply_sum;
        key_switch, key, key_switch_scratch as for multiply_relinearize."""
        if not isinstance(key_switch, KeySwitchPlan) or key_switch.bits != self.bits:
            raise ValueError("key_switch is a KeySwitchPlan of the same word width")
        if key is None or key_switch_scratch is None:
            raise ValueError("null pointer argument")
        terms, x_ptrs, y_ptrs = self._sum_operands(xs, ys, out, 2, count, scratch)
        self._check_buffers([(key, key_switch._key_words(2) if self._cols(count) else 0,
                              "key (D x 2 x key_mod_count x N)")])
        _require_gpu(key_switch_scratch)
        if int(count) > 0 and \
                key_switch_scratch.numel() * key_switch_scratch.element_size() < key_switch.scratch_bytes(count, 2):
            raise ValueError("key_switch_scratch holds fewer than key_switch.scratch_bytes(count, 2) bytes")
        fn = getattr(load_library(), "gpuntt_bfv_plan_multiply_relinearize_sum_u%d" % self.bits)
        _check(fn(self._h, x_ptrs, y_ptrs, terms, key_switch._h, _ptr(key), _ptr(out), int(count),
                  int(bool(input_ntt)), int(bool(output_ntt)), _ptr(scratch), _ptr(key_switch_scratch), _stream(stream)))

    def close(self):
        if self._h:
            getattr(load_library(), "gpuntt_bfv_plan_destroy_u%d" % self.bits)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bfv_slot_maps(n_power):
    """Host (no GPU): (to_position, to_slot), two uint32 arrays of N entries -- where GPU_NTT's output holds slot
    r N/2 + c of the 2 x N/2 BFV slot matrix, and the inverse (include/gpuntt/rns/bfv_encode.cuh has the convention)."""
    if not 1 <= int(n_power) <= 28:
        raise ValueError("Invalid n_power range!")
    to_position = np.empty(1 << int(n_power), dtype=np.uint32)
    to_slot = np.empty_like(to_position)
    _check(load_library().gpuntt_bfv_slot_maps(int(n_power), to_position.ctypes.data_as(ctypes.c_void_p),
                                               to_slot.ctypes.data_as(ctypes.c_void_p)))
    return to_position, to_slot


class BfvBatchEncoder:
    """Extension BfvBatchEncoder<T> (include/gpuntt/rns/bfv_encode.cuh): BFV batching for the plaintext modulus
    `plain_modulus` (a Modulus with t = 1 mod 2N) on a ring of 2^n_power.  forward_table / inverse_table: device tensors
    modulo t as for GPU_NTT / GPU_INTT with X_N_plus, n_inverse = N^-1 mod t.  `workspace`: an optional uint8 device
    tensor of workspace_bytes() bytes owned by the caller.  encode takes slot values to coefficients modulo t, decode
    back; decode needs a caller-owned scratch of scratch_bytes(count) bytes, 256-byte aligned."""

    def __init__(self, plain_modulus, n_power, forward_table, inverse_table, n_inverse, batch_hint=1024, stream=None,
                 workspace=None):
        lib = load_library()
        _require_gpu(workspace, forward_table, inverse_table)
        self.bits, self.n_power, self.plain_modulus = plain_modulus.bits, int(n_power), int(plain_modulus.value)
        for t in (forward_table, inverse_table):
            if t is not None and 1 <= self.n_power <= 28 and (t.element_size() * 8 != self.bits or
                                                              t.numel() < 1 << self.n_power):
                raise ValueError("a table holds N %d-bit words" % self.bits)
        if workspace is not None:
            need = self.workspace_bytes(n_power, self.bits)  # raises for an n_power out of range
            if workspace.numel() * workspace.element_size() < need:
                raise ValueError("workspace holds fewer than workspace_bytes() bytes")
        self._keep = (workspace, forward_table, inverse_table)
        self._h = ctypes.c_void_p()
        fn = getattr(lib, "gpuntt_bfv_encoder_create_u%d" % self.bits)
        _check(fn(ctypes.byref(self._h), plain_modulus.c(), int(n_power), _ptr(forward_table), _ptr(inverse_table),
                  _ct(self.bits)(int(n_inverse)), int(batch_hint), _ptr(workspace), _stream(stream)))

    @staticmethod
    def workspace_bytes(n_power, bits=64):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_bfv_encoder_workspace_bytes_u%d" % bits)(int(n_power), ctypes.byref(out)))
        return int(out.value)

    def scratch_bytes(self, count):
        """the caller-owned scratch of decode: T[count][N], rounded up to 256 bytes"""
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_bfv_encoder_scratch_bytes_u%d" % self.bits)(
            self.n_power, int(count), ctypes.byref(out)))
        return int(out.value)

    @property
    def owns_workspace(self):
        """False: the plan lives in the caller's workspace and has allocated no device memory"""
        return bool(getattr(load_library(), "gpuntt_bfv_encoder_owns_workspace_u%d" % self.bits)(self._h))

    def _check_buffers(self, sized):
        """the library cannot see tensor sizes or types: sized = (tensor, words needed, name) ..."""
        _require_gpu(*[t for t, _, _ in sized])
        for t, words, name in sized:
            if t.element_size() * 8 != self.bits or t.dtype.is_floating_point:
                raise ValueError("a %d-bit BfvBatchEncoder takes %d-bit integer tensors" % (self.bits, self.bits))
            if words > 0 and t.numel() < words:
                raise ValueError("%s needs %d words; got %d" % (name, words, t.numel()))

    def _cols(self, count):
        return (int(count) << self.n_power) if int(count) > 0 else 0

    def encode(self, values, plain, count, stream=None):
        """values T[count][N] (any words, read modulo t, indexed by slot) -> plain T[count][N], the coefficients modulo
        t: one bfv_slot_permute, then the inverse transform modulo t in place"""
        if values is None or plain is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        self._check_buffers(((values, cols, "values (count x N)"), (plain, cols, "plain (count x N)")))
        fn = getattr(load_library(), "gpuntt_bfv_encoder_encode_u%d" % self.bits)
        _check(fn(self._h, _ptr(values), _ptr(plain), int(count), _stream(stream)))

    def decode(self, plain, values, count, scratch, stream=None):
        """plain T[count][N] (canonical coefficients modulo t, left untouched) -> values T[count][N] by slot: the
        forward transform modulo t into the scratch, then one bfv_slot_permute"""
        if plain is None or values is None or scratch is None:
            raise ValueError("null pointer argument")
        cols = self._cols(count)
        self._check_buffers(((plain, cols, "plain (count x N)"), (values, cols, "values (count x N)")))
        _require_gpu(scratch)
        if int(count) >= 0 and scratch.numel() * scratch.element_size() < self.scratch_bytes(count):
            raise ValueError("scratch holds fewer than scratch_bytes(count) bytes")
        fn = getattr(load_library(), "gpuntt_bfv_encoder_decode_u%d" % self.bits)
        _check(fn(self._h, _ptr(plain), _ptr(values), int(count), _ptr(scratch), _stream(stream)))

    def close(self):
        if self._h:
            getattr(load_library(), "gpuntt_bfv_encoder_destroy_u%d" % self.bits)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FourStepPlan:
    """Extension FourStepPlan<T> (include/gpuntt/ntt_4step/ntt_4step.cuh): the Shoup pairs of the n1 / n2 / W
    tables are prepared once; execute() launches the sweeps only.  natural_order False: execute ==
    GPU_4STEP_NTT (n2 x n1 in, n1 x n2 out); True: == GPU_4STEP_NTT_NaturalOrder (device_in is scratch).
    `cfg` is an ntt4step_configuration (n_power, ntt_type, mod_inverse, stream of the preparation);
    `workspace` an optional uint8 device tensor of workspace_bytes() bytes owned by the caller."""

    def __init__(self, n1_root_of_unity_table, n2_root_of_unity_table, W_root_of_unity_table, modulus, cfg,
                 natural_order=False, batch_hint=1, workspace=None):
        lib = load_library()
        _require_gpu(n1_root_of_unity_table, n2_root_of_unity_table, W_root_of_unity_table)
        self.bits = modulus.bits
        self.n_power, self.ntt_type, self.natural_order = cfg.n_power, cfg.ntt_type, bool(natural_order)
        self._keep = (n1_root_of_unity_table, n2_root_of_unity_table, W_root_of_unity_table, workspace)
        self._h = ctypes.c_void_p()
        fn = getattr(lib, "gpuntt_4step_plan_create_u%d" % self.bits)
        _check(fn(ctypes.byref(self._h), _ptr(n1_root_of_unity_table), _ptr(n2_root_of_unity_table),
                  _ptr(W_root_of_unity_table), modulus.c(), cfg.n_power, cfg.ntt_type,
                  _ct(self.bits)(cfg.mod_inverse), int(self.natural_order), int(batch_hint), _ptr(workspace),
                  _stream(cfg.stream)))

    @staticmethod
    def workspace_bytes(n_power, bits=64):
        out = ctypes.c_uint64()
        _check(getattr(load_library(), "gpuntt_4step_plan_workspace_bytes_u%d" % bits)(n_power, ctypes.byref(out)))
        return int(out.value)

    @property
    def fast_path(self):
        return bool(getattr(load_library(), "gpuntt_4step_plan_fast_path_u%d" % self.bits)(self._h))

    def execute(self, device_in, device_out, batch_size, stream=None):
        _require_gpu(device_in, device_out)
        fn = getattr(load_library(), "gpuntt_4step_plan_execute_u%d" % self.bits)
        _check(fn(self._h, _ptr(device_in), _ptr(device_out), int(batch_size), _stream(stream)))

    def close(self):
        if self._h:
            getattr(load_library(), "gpuntt_4step_plan_destroy_u%d" % self.bits)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def GPU_GeneratePowerTable(device_out, base, modulus, log_count, bit_reversed=True, stream=None):
    """Extension: device_out[k] = base^(bitreverse(k, log_count) if bit_reversed else k), k < 2^log_count -- the
    device-order root tables of GPU_NTT / GPU_INTT / the 4-step n1, n2 slots, built on the device."""
    _require_gpu(device_out)
    fn = getattr(load_library(), "gpuntt_generate_power_table_u%d" % modulus.bits)
    _check(fn(_ptr(device_out), _ct(modulus.bits)(base), modulus.c(), int(log_count), int(bool(bit_reversed)),
              _stream(stream)))


def GPU_Generate4StepW(device_W, root, modulus, n_power, ntt_type=FORWARD, stream=None):
    """Extension: the 4-step W matrix on the device: FORWARD W[i*n2+j] = root^(bitreverse(i)*j) (root_of_unity),
    INVERSE W[i*n2+j] = root^(bitreverse(j)*i) (inverse_root_of_unity)."""
    _require_gpu(device_W)
    fn = getattr(load_library(), "gpuntt_generate_4step_w_u%d" % modulus.bits)
    _check(fn(_ptr(device_W), _ct(modulus.bits)(root), modulus.c(), int(n_power), int(ntt_type), _stream(stream)))


def release_workspaces():
    """GPU_NTT_ReleaseWorkspaces(): frees the library-owned twiddle scratch of the drop-in calls."""
    _check(load_library().gpuntt_release_workspaces())


def operator_gpu(op, a, b, modulus):
    """diagnostic: OPERATOR_GPU<T>::{add, sub, mult, reduce, reduce(signed), centered_reduction}
    (op 0..5) elementwise on device tensors; returns a new tensor"""
    import torch
    lib = load_library()
    _require_gpu(a, b)
    out = torch.empty_like(a)
    fn = getattr(lib, "gpuntt_operator_gpu_u%d" % modulus.bits)
    _check(fn(int(op), _ptr(a), _ptr(b), _ptr(out), modulus.c(), ctypes.c_uint64(a.numel()), _stream(None)))
    return out


def debug_recip_norm(q):
    """diagnostic: the preparation kernels' normalised reciprocal of every word of the device tensor q; returns a new tensor"""
    import torch
    _require_gpu(q)
    out = torch.empty_like(q)
    fn = getattr(load_library(), "gpuntt_debug_recip_norm_u%d" % (q.element_size() * 8))
    _check(fn(_ptr(q), _ptr(out), ctypes.c_uint64(q.numel()), _stream(None)))
    return out


def butterfly_unit(u, v, roots, modulus, gentleman_sande=False):
    """diagnostic: the public device helpers CooleyTukeyUnit / GentlemanSandeUnit (reference ntt.cuh:69-92) applied to
    the pairs (u[i], v[i]) with roots[i], in place on the device tensors"""
    lib = load_library()
    _require_gpu(u, v, roots)
    fn = getattr(lib, "gpuntt_butterfly_unit_u%d" % modulus.bits)
    _check(fn(int(bool(gentleman_sande)), _ptr(u), _ptr(v), _ptr(roots), modulus.c(), ctypes.c_uint64(u.numel()),
              _stream(None)))


# ------------------------------------------------------------------ multi-GPU batch shard
def shard_range(batch_size, rank, world_size, mod_count=1):
    """Rank r of G owns polynomials [lo, hi) of the batch; shards are aligned to mod_count so
    the local p % mod_count equals the global one.  Polynomials are
    independent: no data-path collective exists anywhere in a transform."""
    if batch_size % mod_count:
        raise ValueError("batch_size must be a multiple of mod_count")
    groups = batch_size // mod_count
    lo = (groups * rank) // world_size
    hi = (groups * (rank + 1)) // world_size
    return lo * mod_count, hi * mod_count
