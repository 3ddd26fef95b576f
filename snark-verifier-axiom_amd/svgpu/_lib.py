"""ctypes binding of libsvgpu.so (include/svgpu.h).

The library is built in-tree (``make -C snark-verifier-axiom_amd`` -> ``build/libsvgpu.so``).
There is no fallback: if the shared object is missing this module raises at import time, and
compute calls without a GPU raise :class:`DeviceError` (status SV_ERR_DEVICE).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_size_t, c_uint8, c_uint16, c_uint32,
                    c_uint64, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVGPU_LIB", os.path.join(os.path.dirname(_HERE), "build", "libsvgpu.so"))

SV_CANONICAL = 0
SV_MONTGOMERY = 1

SV_OK, SV_ERR_EMPTY, SV_ERR_LEN, SV_ERR_ARG, SV_ERR_DEVICE, SV_ERR_OOM = range(6)

SV_OPEN_BATCH_MAX = 4096  # polynomials per batched opening
SV_EVAL_POINTS_MAX = 16   # points per evaluation call, roots per division, points per SHPLONK set

SV_NTT_MAX_LOG = 26        # log2 of the longest transform
SV_NTT_FORWARD = 0
SV_NTT_INVERSE = 1
SV_EXT_LOG_MAX = 8         # log2 of the widest extension of coset_lde / quotient_coeffs
SV_TERMS_COLUMNS_MAX = 64  # permutation columns (and z columns) per permutation_terms call
SV_TERMS_LOOKUPS_MAX = 16  # lookups per lookup_terms call
SV_LOOKUP_BATCH_MAX = 16   # lookups per lookup_permute_batch call
SV_LOOKUP_TABLES_SORTED = 1  # lookup_permute_batch flag: every table is already sorted

# opcodes of an expression program (sv_fr_expr_op.op)
(SV_EXPR_COLUMN, SV_EXPR_CONST, SV_EXPR_NEG, SV_EXPR_ADD, SV_EXPR_SUB, SV_EXPR_RSUB, SV_EXPR_MUL, SV_EXPR_FOLD,
 SV_EXPR_STORE) = range(9)
SV_EXPR_OPS_MAX = 4096     # ops per program
SV_EXPR_COLUMNS_MAX = 256  # columns a program can name
SV_EXPR_CONSTS_MAX = 256   # constants (and challenges) a program can name
SV_EXPR_STORES_MAX = 16    # columns a program can write with STORE
SV_EXPR_STACK_MAX = 8      # the deepest operand stack

SV_FACTOR_PLAIN = 0        # f[i] = x[i] + c
SV_FACTOR_COLUMN = 1       # f[i] = x[i] + s*y[i] + c
SV_FACTOR_IDENTITY = 2     # f[i] = x[i] + s*omega^i + c
SV_PRODUCT_FACTORS_MAX = 16  # factors per side of a grand product

SV_ENC_HALO2_COMPRESSED = 0
SV_ENC_EVM = 1


class SvError(RuntimeError):
    status = -1


class EmptyError(SvError):
    status = SV_ERR_EMPTY


class LengthError(SvError):
    status = SV_ERR_LEN


class ArgumentError(SvError):
    status = SV_ERR_ARG


class DeviceError(SvError):
    status = SV_ERR_DEVICE


class OutOfMemoryError(SvError):
    status = SV_ERR_OOM


_ERRORS = {c.status: c for c in (EmptyError, LengthError, ArgumentError, DeviceError, OutOfMemoryError)}


class sv_fe(Structure):
    _fields_ = [("l", c_uint64 * 4)]


class sv_g1_affine(Structure):
    _fields_ = [("x", sv_fe), ("y", sv_fe)]


class sv_g1_jacobian(Structure):
    _fields_ = [("x", sv_fe), ("y", sv_fe), ("z", sv_fe)]


class sv_fq2(Structure):
    _fields_ = [("c0", sv_fe), ("c1", sv_fe)]


class sv_g2_affine(Structure):
    _fields_ = [("x", sv_fq2), ("y", sv_fq2)]


class sv_fq12(Structure):
    _fields_ = [("c", sv_fq2 * 6)]


class sv_shplonk_set(Structure):
    _fields_ = [("first_poly", c_uint32), ("num_polys", c_uint32), ("first_point", c_uint32),
                ("num_points", c_uint32)]


class sv_fr_factor(Structure):
    _fields_ = [("d_x", c_void_p), ("d_y", c_void_p), ("s", sv_fe), ("c", sv_fe), ("kind", c_uint32)]


class sv_fr_lookup(Structure):
    _fields_ = [("d_z", c_void_p), ("d_permuted_input", c_void_p), ("d_permuted_table", c_void_p),
                ("d_input", c_void_p), ("d_table", c_void_p)]


class sv_fr_expr_op(Structure):
    _fields_ = [("op", c_uint8), ("zero", c_uint8), ("index", c_uint16), ("rotation", c_int32)]


class sv_msm_stats(Structure):
    _fields_ = [
        ("total_ms", c_float), ("digits_ms", c_float), ("sort_ms", c_float), ("accumulate_ms", c_float),
        ("fixup_ms", c_float), ("reduce_ms", c_float), ("host_ms", c_float),
        ("window_bits", c_uint32), ("num_windows", c_uint32), ("accumulate_launch_units", c_uint32),
        ("entries", c_uint64), ("accumulate_span_ms", c_float), ("accumulate_launches", c_uint32),
    ]


# (name, restype, argtypes) -- one row per prototype in include/svgpu.h
PROTOTYPES = [
    ("sv_init", c_int, [c_int]),
    ("sv_device_count", c_int, []),
    ("sv_last_error", c_char_p, []),
    ("sv_version", c_char_p, []),
    ("sv_bn254_g1_msm", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(sv_g1_affine)]),
    ("sv_bn254_g1_msm_refs", c_int, [c_void_p, c_size_t, c_int, c_int, POINTER(sv_g1_affine)]),
    ("sv_bn254_g1_msm_device", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p, POINTER(sv_g1_jacobian)]),
    ("sv_bn254_g1_fold", c_int, [c_void_p, c_size_t, POINTER(sv_g1_affine), c_int]),
    ("sv_bn254_kzg_decide", c_int, [POINTER(sv_g2_affine), POINTER(sv_g2_affine), c_void_p, c_void_p, c_size_t,
                                     c_int, c_int, POINTER(c_int32)]),
    ("sv_bn254_kzg_decide_device", c_int, [POINTER(sv_g2_affine), POINTER(sv_g2_affine), c_void_p, c_void_p,
                                            c_size_t, c_int, c_int, c_void_p, POINTER(c_int32), c_void_p, c_void_p]),
    ("sv_bn254_kzg_accumulate", c_int, [c_void_p, c_void_p, c_size_t, POINTER(sv_fe), c_int, c_int,
                                         POINTER(sv_g1_affine), POINTER(sv_g1_affine)]),
    ("sv_bn254_kzg_create_proof", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(sv_g1_affine),
                                           POINTER(sv_g1_affine), c_void_p, c_void_p]),
    ("sv_bn254_g1_msm_batch", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    ("sv_bn254_g1_msm_batch_device", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_int, c_int,
                                              c_void_p, c_void_p]),
    ("sv_bn254_g1_table_create", c_int, [c_void_p, c_size_t, c_int, c_int, POINTER(c_uint64)]),
    ("sv_bn254_g1_table_destroy", c_int, [c_uint64]),
    ("sv_bn254_g1_msm_batch_table", c_int, [c_uint64, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    ("sv_bn254_g1_msm_batch_table_device", c_int, [c_uint64, c_void_p, c_void_p, c_void_p, c_size_t, c_int,
                                                    c_void_p, c_void_p]),
    ("sv_bn254_g1_table_device", c_int, [c_uint64, POINTER(c_int)]),
    ("sv_bn254_g1_msm_batch_indexed_device", c_int, [c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_void_p,
                                                      c_size_t, c_size_t, c_int, c_int, c_void_p, c_void_p]),
    ("sv_bn254_g1_bases_create", c_int, [c_void_p, c_size_t, c_int, c_int, POINTER(c_uint64)]),
    ("sv_bn254_g1_bases_create_device", c_int, [c_void_p, c_size_t, c_int, c_int, c_void_p, POINTER(c_uint64)]),
    ("sv_bn254_g1_bases_destroy", c_int, [c_uint64]),
    ("sv_bn254_g1_bases_info", c_int, [c_uint64, POINTER(c_uint64), POINTER(c_int), POINTER(c_uint64)]),
    ("sv_bn254_g1_msm_bases", c_int, [c_uint64, c_size_t, c_void_p, c_size_t, c_int, POINTER(sv_g1_affine)]),
    ("sv_bn254_g1_msm_bases_device", c_int, [c_uint64, c_size_t, c_void_p, c_size_t, c_int, c_void_p,
                                              POINTER(sv_g1_jacobian)]),
    ("sv_bn254_fr_poly_div_linear_device", c_int, [c_void_p, c_size_t, POINTER(sv_fe), c_int, c_int, c_void_p,
                                                    c_void_p, POINTER(sv_fe)]),
    ("sv_bn254_kzg_open", c_int, [c_uint64, c_size_t, c_void_p, c_size_t, POINTER(sv_fe), c_int, POINTER(sv_fe),
                                   POINTER(sv_g1_affine)]),
    ("sv_bn254_kzg_open_device", c_int, [c_uint64, c_size_t, c_void_p, c_size_t, POINTER(sv_fe), c_int, c_void_p,
                                          POINTER(sv_fe), POINTER(sv_g1_jacobian)]),
    ("sv_bn254_fr_poly_combine_eval_device", c_int, [c_void_p, c_void_p, c_size_t, POINTER(sv_fe), POINTER(sv_fe),
                                                      c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("sv_bn254_kzg_open_batch_device", c_int, [c_uint64, c_size_t, c_void_p, c_void_p, c_size_t, POINTER(sv_fe),
                                                POINTER(sv_fe), c_int, c_void_p, c_void_p, POINTER(sv_g1_jacobian)]),
    ("sv_bn254_fr_poly_eval_points_device", c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_int,
                                                     c_void_p, c_void_p]),
    ("sv_bn254_fr_poly_div_roots_device", c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_int, c_void_p,
                                                   c_void_p]),
    ("sv_bn254_shplonk_work_elems", c_int, [c_size_t, c_size_t, POINTER(c_uint64)]),
    ("sv_bn254_shplonk_quotient_device", c_int, [c_uint64, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                                  c_void_p, c_size_t, POINTER(sv_fe), POINTER(sv_fe), c_int, c_void_p,
                                                  c_void_p, c_uint64, POINTER(sv_g1_jacobian)]),
    ("sv_bn254_shplonk_witness_device", c_int, [c_uint64, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p,
                                                 POINTER(sv_fe), POINTER(sv_fe), c_int, c_void_p, c_void_p, c_uint64,
                                                 POINTER(sv_g1_jacobian)]),
    ("sv_bn254_fr_root_of_unity", c_int, [c_uint32, c_int, POINTER(sv_fe)]),
    ("sv_bn254_fr_ntt_device", c_int, [c_void_p, c_void_p, c_uint32, c_size_t, c_int, c_void_p, c_int, c_int,
                                        c_void_p]),
    ("sv_bn254_fr_coset_lde_device", c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_size_t, c_void_p, c_int,
                                              c_int, c_void_p]),
    ("sv_bn254_fr_quotient_coeffs_device", c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_size_t, c_void_p,
                                                    c_int, c_int, c_void_p]),
    ("sv_bn254_fr_permutation_terms_device", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p,
                                                      c_void_p, c_void_p, c_void_p, POINTER(sv_fe), POINTER(sv_fe),
                                                      POINTER(sv_fe), POINTER(sv_fe), c_int32, c_void_p, c_void_p,
                                                      c_uint32, c_uint32, c_int, c_int, c_void_p]),
    ("sv_bn254_fr_lookup_terms_device", c_int, [c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, POINTER(sv_fe),
                                                 POINTER(sv_fe), POINTER(sv_fe), c_void_p, c_void_p, c_uint32, c_uint32,
                                                 c_int, c_int, c_void_p]),
    ("sv_bn254_fr_expressions_device", c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p,
                                                c_size_t, POINTER(sv_fe), c_void_p, c_void_p, c_uint32, c_uint32, c_int,
                                                c_int, c_void_p]),
    ("sv_bn254_fr_grand_product_device", c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, POINTER(sv_fe),
                                                  POINTER(sv_fe), c_int, c_void_p, POINTER(sv_fe), c_int, c_void_p]),
    ("sv_bn254_fr_batch_invert_device", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    ("sv_bn254_fr_sort_device", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    ("sv_bn254_fr_lookup_permute_device", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p,
                                                   POINTER(c_uint64), c_int, c_void_p]),
    ("sv_bn254_fr_lookup_permute_batch_device", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_int, c_uint32,
                                                         c_void_p, c_void_p, POINTER(c_uint64), POINTER(c_uint64),
                                                         c_int, c_void_p]),
    ("sv_bn254_poseidon_permute", c_int, [c_void_p, c_size_t, c_int, c_int]),
    ("sv_bn254_poseidon_permute_device", c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    ("sv_bn254_poseidon_squeeze", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    ("sv_bn254_poseidon_squeeze_device", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p,
                                                  c_int, c_void_p]),
    ("sv_bn254_g1_decode", c_int, [c_void_p, c_size_t, c_int, c_int, c_void_p, POINTER(ctypes.c_int64)]),
    ("sv_bn254_g1_decode_device", c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p,
                                           POINTER(ctypes.c_int64)]),
    ("sv_bn254_kzg_accumulators_from_limbs", c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p,
                                                      POINTER(ctypes.c_int64)]),
    ("sv_bn254_kzg_decide_eip197", c_int, [c_void_p, c_size_t, c_int, POINTER(c_int32)]),
    ("sv_gen_scalars_device", c_int, [c_void_p, c_size_t, c_uint64, c_uint64, c_int, c_int, c_void_p]),
    ("sv_gen_bases_device", c_int, [c_void_p, c_size_t, c_uint64, c_uint64, c_int, c_int, c_void_p]),
    ("sv_msm_last_stats", c_int, [POINTER(sv_msm_stats)]),
    ("sv_kzg_last_kernel_ms", c_int, [POINTER(c_float)]),
]


def _check_fresh():
    """The library must have been linked from the sources beside it (build/SOURCES.sha256, written
    by the Makefile): a prebuilt .so that travelled with a changed tree raises here.
    SVGPU_ALLOW_STALE=1 skips the check (e.g. an A/B library in another directory)."""
    if os.environ.get("SVGPU_ALLOW_STALE") == "1" or "SVGPU_LIB" in os.environ:
        return
    from ._srchash import source_hash
    stamp = os.path.join(os.path.dirname(LIB_PATH), "SOURCES.sha256")
    want = source_hash()
    have = open(stamp).read().strip() if os.path.exists(stamp) else "(no stamp)"
    if have != want:
        raise ImportError(f"{LIB_PATH} was not built from the current sources (stamp {have[:16]}, sources "
                          f"{want[:16]}): rebuild with `make -C snark-verifier-axiom_amd`")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libsvgpu.so not found at {LIB_PATH}: build it with `make -C snark-verifier-axiom_amd` "
            "(there is no CPU fallback)")
    _check_fresh()
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in PROTOTYPES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def last_error() -> str:
    msg = lib.sv_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str = "") -> None:
    if rc == SV_OK:
        return
    cls = _ERRORS.get(rc, SvError)
    raise cls(f"{what}: status {rc}: {last_error()}")
