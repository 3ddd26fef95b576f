"""Device-resident (HBM) entry points over torch tensors.

PyTorch is plumbing here: it owns device memory and the stream; the work is libsvgpu's HIP
kernels.  Tensors are int64 views of the C-ABI layouts: bases (n, 8), scalars (n, 4).
"""
from __future__ import annotations

import copy
import ctypes
from collections import namedtuple
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import encoding as enc


def _stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _dev_index(t: torch.Tensor) -> int:
    if t.device.type != "cuda":
        raise _lib.DeviceError("tensor must live on a GPU (cuda/HIP device)")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def empty_bases(n: int, device) -> torch.Tensor:
    return torch.empty((n, 8), dtype=torch.int64, device=device)


def empty_scalars(n: int, device) -> torch.Tensor:
    return torch.empty((n, 4), dtype=torch.int64, device=device)


def gen_bases(t: torch.Tensor, seed: int, start: int = 0, form: int = _lib.SV_MONTGOMERY) -> torch.Tensor:
    d = _dev_index(t)
    _lib.check(_lib.lib.sv_gen_bases_device(t.data_ptr(), t.shape[0], seed, start, form, d,
                                            _stream_handle(t.device)), "sv_gen_bases_device")
    return t


def gen_scalars(t: torch.Tensor, seed: int, start: int = 0, form: int = _lib.SV_MONTGOMERY) -> torch.Tensor:
    d = _dev_index(t)
    _lib.check(_lib.lib.sv_gen_scalars_device(t.data_ptr(), t.shape[0], seed, start, form, d,
                                              _stream_handle(t.device)), "sv_gen_scalars_device")
    return t


def msm_partial(bases: torch.Tensor, scalars: torch.Tensor, form: int = _lib.SV_MONTGOMERY) -> Tuple[int, int, int]:
    """One device's MSM over HBM-resident inputs -> canonical Jacobian (X, Y, Z) on the host."""
    if bases.shape[0] != scalars.shape[0]:
        raise ValueError("bases and scalars differ in length")
    d = _dev_index(bases)
    out = _lib.sv_g1_jacobian()
    _lib.check(_lib.lib.sv_bn254_g1_msm_device(bases.data_ptr(), scalars.data_ptr(), bases.shape[0], form, d,
                                               _stream_handle(bases.device), ctypes.byref(out)),
               "sv_bn254_g1_msm_device")
    return enc.jacobian_from_struct(out)


def msm(bases: torch.Tensor, scalars: torch.Tensor, form: int = _lib.SV_MONTGOMERY):
    """One device's MSM -> affine point (canonical ints; None = identity).  The Jacobian partial
    goes straight from sv_bn254_g1_msm_device into sv_bn254_g1_fold (no Python-int round trip)."""
    if bases.shape[0] != scalars.shape[0]:
        raise ValueError("bases and scalars differ in length")
    d = _dev_index(bases)
    part = _lib.sv_g1_jacobian()
    _lib.check(_lib.lib.sv_bn254_g1_msm_device(bases.data_ptr(), scalars.data_ptr(), bases.shape[0], form, d,
                                               _stream_handle(bases.device), ctypes.byref(part)),
               "sv_bn254_g1_msm_device")
    out = _lib.sv_g1_affine()
    _lib.check(_lib.lib.sv_bn254_g1_fold(ctypes.byref(part), 1, ctypes.byref(out), _lib.SV_CANONICAL),
               "sv_bn254_g1_fold")
    return enc.g1_from_struct(out)


def poly_div_linear_device(coeffs: torch.Tensor, z: int, form: int = _lib.SV_MONTGOMERY, quotient: bool = True,
                           out: torch.Tensor = None) -> Tuple[int, Optional[torch.Tensor]]:
    """(p - p(z)) / (X - z) for the HBM-resident coefficients of p ((n, 4) int64 limbs in `form`; z a
    canonical int) -> (p(z) as a canonical int, the n - 1 quotient coefficients in `form`, or None
    with quotient=False: evaluate only).  `out` (at least n - 1 rows) must not overlap coeffs."""
    d = _dev_index(coeffs)
    coeffs = coeffs.contiguous()
    n = coeffs.shape[0]
    if quotient and out is None:
        out = torch.empty((max(n - 1, 1), 4), dtype=torch.int64, device=coeffs.device)
    elif quotient and (out.device != coeffs.device or out.dtype != torch.int64 or not out.is_contiguous()
                       or out.dim() != 2 or out.shape[1] != 4 or out.shape[0] < n - 1):
        raise _lib.LengthError(f"poly_div: out must be a contiguous (>= {n - 1}, 4) int64 tensor on {coeffs.device}")
    zs, ev = enc.fr_struct(z, form), _lib.sv_fe()
    _lib.check(_lib.lib.sv_bn254_fr_poly_div_linear_device(coeffs.data_ptr(), n, ctypes.byref(zs), form, d,
                                                           _stream_handle(coeffs.device),
                                                           out.data_ptr() if quotient else None, ctypes.byref(ev)),
               "sv_bn254_fr_poly_div_linear_device")
    return enc.fr_from_struct(ev, form), (out[:n - 1] if quotient else None)


def batch_tables(polys):
    """The host arrays of a batched call: (tensors kept alive, c_void_p[m] device pointers,
    c_uint64[m] lengths) for a list of (n_j, 4) int64 tensors on one GPU."""
    keep = []
    for p in polys:
        if p.device.type != "cuda":
            raise _lib.DeviceError("tensor must live on a GPU (cuda/HIP device)")
        if p.dtype != torch.int64 or p.dim() != 2 or p.shape[1] != 4:
            raise _lib.ArgumentError("a polynomial is an (n, 4) int64 tensor of limbs")
        if keep and p.device != keep[0].device:
            raise _lib.ArgumentError("the polynomials of a batch live on one device")
        keep.append(p.contiguous())
    m = len(keep)
    ptrs = (ctypes.c_void_p * max(m, 1))(*[p.data_ptr() for p in keep])
    lens = (ctypes.c_uint64 * max(m, 1))(*[p.shape[0] for p in keep])
    return keep, ptrs, lens


def combine_eval_pointers(ptrs, lens, m: int, z: int, v: int, form: int, device: int, stream, combined_ptr) -> List[int]:
    """sv_bn254_fr_poly_combine_eval_device over raw host arrays of device pointers and lengths
    (what poly_combine_eval_device builds from tensors) -> the m evaluations as canonical ints."""
    zs, vs = enc.fr_struct(z, form), enc.fr_struct(v, form)
    ev = (_lib.sv_fe * max(m, 1))()
    _lib.check(_lib.lib.sv_bn254_fr_poly_combine_eval_device(ptrs, lens, m, ctypes.byref(zs), ctypes.byref(vs), form,
                                                             device, stream, combined_ptr, ev),
               "sv_bn254_fr_poly_combine_eval_device")
    return [enc.fr_from_struct(ev[j], form) for j in range(m)]


def poly_combine_eval_device(polys, z: int, v: int, form: int = _lib.SV_MONTGOMERY, combined: bool = True,
                             out: torch.Tensor = None) -> Tuple[List[int], Optional[torch.Tensor]]:
    """One GWC19 point set without the witness: for the HBM-resident polynomials p_j ((n_j, 4) int64
    limbs in `form`; z and v canonical ints) -> ([p_j(z)] as canonical ints, c = sum_j v^j p_j as
    N = max n_j rows in `form`, or None with combined=False: evaluate only).  A shorter polynomial is
    zero past its end; `out` (at least N rows) must not overlap a polynomial."""
    keep, ptrs, lens = batch_tables(polys)
    m = len(keep)
    n = max((p.shape[0] for p in keep), default=0)
    d, stream, dev = 0, None, None
    if m:
        dev = keep[0].device
        d, stream = _dev_index(keep[0]), _stream_handle(dev)
    if combined and out is None and m:
        out = torch.empty((max(n, 1), 4), dtype=torch.int64, device=dev)
    elif combined and m and (out.device != dev or out.dtype != torch.int64 or not out.is_contiguous()
                             or out.dim() != 2 or out.shape[1] != 4 or out.shape[0] < n):
        raise _lib.LengthError(f"poly_combine_eval: out must be a contiguous (>= {n}, 4) int64 tensor on {dev}")
    evals = combine_eval_pointers(ptrs, lens, m, z, v, form, d, stream,
                                  out.data_ptr() if combined and out is not None else None)
    return evals, (out[:n] if combined else None)


def fe_array(values, form: int):
    """A host array of sv_fe (at least one element) holding the canonical ints `values` in `form`."""
    arr = (_lib.sv_fe * max(len(values), 1))()
    for k, x in enumerate(values):
        arr[k] = enc.fr_struct(x, form)
    return arr


def eval_points_pointers(ptrs, lens, m: int, points, form: int, device: int, stream) -> List[List[int]]:
    """sv_bn254_fr_poly_eval_points_device over raw host arrays of device pointers and lengths ->
    [[p_j(x_k) for k] for j] as canonical ints."""
    K = len(points)
    ev = (_lib.sv_fe * max(m * K, 1))()
    _lib.check(_lib.lib.sv_bn254_fr_poly_eval_points_device(ptrs, lens, m, fe_array(points, form), K, form, device,
                                                            stream, ev),
               "sv_bn254_fr_poly_eval_points_device")
    return [[enc.fr_from_struct(ev[j * K + k], form) for k in range(K)] for j in range(m)]


def poly_eval_points_device(polys, points, form: int = _lib.SV_MONTGOMERY) -> List[List[int]]:
    """Every p_j(x_k) for the HBM-resident polynomials p_j ((n_j, 4) int64 limbs in `form`) and the
    points x_k (canonical ints, at most SV_EVAL_POINTS_MAX; repeats allowed) in one pass that reads
    each polynomial once -> [[p_j(x_k) for k] for j], canonical ints."""
    keep, ptrs, lens = batch_tables(polys)
    d, stream = (_dev_index(keep[0]), _stream_handle(keep[0].device)) if keep else (0, None)
    return eval_points_pointers(ptrs, lens, len(keep), list(points), form, d, stream)


def poly_div_roots_device(coeffs: torch.Tensor, roots, form: int = _lib.SV_MONTGOMERY,
                          out: torch.Tensor = None) -> torch.Tensor:
    """The quotient of p by prod_k (X - x_k), remainder dropped, for the HBM-resident coefficients of
    p ((n, 4) int64 limbs in `form`) and the roots x_k (canonical ints, K < n) -> n - K rows in `form`.
    `out` (at least n - K rows) must not overlap coeffs."""
    d = _dev_index(coeffs)
    coeffs = coeffs.contiguous()
    roots = list(roots)
    n, K = coeffs.shape[0], len(roots)
    if out is None:
        out = torch.empty((max(n - K, 1), 4), dtype=torch.int64, device=coeffs.device)
    elif (out.device != coeffs.device or out.dtype != torch.int64 or not out.is_contiguous() or out.dim() != 2
          or out.shape[1] != 4 or out.shape[0] < n - K):
        raise _lib.LengthError(f"poly_div_roots: out must be a contiguous (>= {n - K}, 4) int64 tensor on {coeffs.device}")
    _lib.check(_lib.lib.sv_bn254_fr_poly_div_roots_device(coeffs.data_ptr(), n, fe_array(roots, form), K, form, d,
                                                          _stream_handle(coeffs.device), out.data_ptr()),
               "sv_bn254_fr_poly_div_roots_device")
    return out[:max(n - K, 0)]


def ntt_device(data: torch.Tensor, inverse: bool = False, shift: Optional[int] = None,
               form: int = _lib.SV_MONTGOMERY, out: torch.Tensor = None) -> torch.Tensor:
    """NTT of HBM-resident Fr data: an (n, 4) int64 tensor of limbs in `form` is one transform, a
    (count, n, 4) tensor `count` transforms back to back; n is a power of two (else LengthError).
    Forward: out[j] = sum_i data[i] (shift omega^j)^i with omega = root_of_unity(log2 n); inverse=True
    is its exact inverse; natural order on both sides.  shift: a canonical int, None = 1.
    out=None allocates, out=data is in place; any other `out` (same shape) must not overlap data."""
    d = _dev_index(data)
    if data.dtype != torch.int64 or data.dim() not in (2, 3) or data.shape[-1] != 4 or not data.is_contiguous():
        raise _lib.ArgumentError("ntt: data is a contiguous (n, 4) or (count, n, 4) int64 tensor of limbs")
    n = data.shape[-2]
    count = data.shape[0] if data.dim() == 3 else 1
    if n == 0 or n & (n - 1):
        raise _lib.LengthError(f"ntt: {n} rows per transform is not a power of two")
    if out is None:
        out = torch.empty_like(data)
    elif (out.device != data.device or out.dtype != torch.int64 or not out.is_contiguous()
          or out.shape != data.shape):
        raise _lib.LengthError(f"ntt: out must be a contiguous {tuple(data.shape)} int64 tensor on {data.device}")
    gs = enc.fr_struct(shift, form) if shift is not None else None
    _lib.check(_lib.lib.sv_bn254_fr_ntt_device(data.data_ptr(), out.data_ptr(), n.bit_length() - 1, count,
                                               _lib.SV_NTT_INVERSE if inverse else _lib.SV_NTT_FORWARD,
                                               ctypes.byref(gs) if gs is not None else None, form, d,
                                               _stream_handle(data.device)),
               "sv_bn254_fr_ntt_device")
    return out


def coset_lde_device(coeffs: torch.Tensor, log_ext: int, shift: Optional[int] = None,
                     form: int = _lib.SV_MONTGOMERY, out: torch.Tensor = None) -> torch.Tensor:
    """Coset low-degree extension of HBM-resident coefficients: an (n, 4) int64 tensor of limbs in
    `form` is one polynomial, a (count, n, 4) tensor `count` polynomials back to back; n is a power of
    two (else LengthError).  out[j] = sum_i coeffs[i] (shift omega_K^j)^i for j < 2^log_ext n, with
    omega_K = root_of_unity(log2 n + log_ext), natural order: (2^log_ext n, 4) or (count, 2^log_ext n,
    4).  shift: a canonical int, None = 1.  out=None allocates; an `out` must not overlap coeffs."""
    d = _dev_index(coeffs)
    if coeffs.dtype != torch.int64 or coeffs.dim() not in (2, 3) or coeffs.shape[-1] != 4 or not coeffs.is_contiguous():
        raise _lib.ArgumentError("coset_lde: coeffs is a contiguous (n, 4) or (count, n, 4) int64 tensor of limbs")
    n = coeffs.shape[-2]
    count = coeffs.shape[0] if coeffs.dim() == 3 else 1
    if n == 0 or n & (n - 1):
        raise _lib.LengthError(f"coset_lde: {n} coefficients per polynomial is not a power of two")
    if not 0 <= log_ext <= _lib.SV_EXT_LOG_MAX:
        raise _lib.LengthError(f"coset_lde: log_ext = {log_ext} is not in 0 .. {_lib.SV_EXT_LOG_MAX}")
    shape = tuple(coeffs.shape[:-2]) + (n << log_ext, 4)
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=coeffs.device)
    elif (out.device != coeffs.device or out.dtype != torch.int64 or not out.is_contiguous()
          or tuple(out.shape) != shape):
        raise _lib.LengthError(f"coset_lde: out must be a contiguous {shape} int64 tensor on {coeffs.device}")
    gs = enc.fr_struct(shift, form) if shift is not None else None
    _lib.check(_lib.lib.sv_bn254_fr_coset_lde_device(coeffs.data_ptr(), out.data_ptr(), n.bit_length() - 1, log_ext,
                                                     count, ctypes.byref(gs) if gs is not None else None, form, d,
                                                     _stream_handle(coeffs.device)),
               "sv_bn254_fr_coset_lde_device")
    return out


def quotient_coeffs_device(numer: torch.Tensor, log_n: int, pieces: int, shift: int,
                           form: int = _lib.SV_MONTGOMERY, out: torch.Tensor = None) -> torch.Tensor:
    """The quotient's coefficients from the numerator's evaluations on the extended coset: numer is a
    (2^K, 4) int64 tensor of limbs in `form`, numer[j] = N(shift omega_K^j); with n = 2^log_n the
    result is the first pieces n coefficients of the polynomial that takes N_j / ((shift omega_K^j)^n
    - 1) there: (pieces n, 4), `pieces` blocks of n.  shift: a canonical int (required).  out=None
    allocates, out=numer is in place (the first pieces n rows of numer are returned); any other `out`
    (at least pieces n rows) must not overlap numer, and nothing past its first pieces n rows is
    written."""
    d = _dev_index(numer)
    if numer.dtype != torch.int64 or numer.dim() != 2 or numer.shape[-1] != 4 or not numer.is_contiguous():
        raise _lib.ArgumentError("quotient_coeffs: numer is a contiguous (2^K, 4) int64 tensor of limbs")
    N = numer.shape[0]
    if N == 0 or N & (N - 1):
        raise _lib.LengthError(f"quotient_coeffs: {N} evaluations is not a power of two")
    K = N.bit_length() - 1
    if not 0 <= log_n <= K:
        raise _lib.LengthError(f"quotient_coeffs: log_n = {log_n} is not in 0 .. {K}")
    if pieces < 0 or pieces > N >> log_n:
        raise _lib.LengthError(f"quotient_coeffs: pieces = {pieces}: the extended domain holds {N >> log_n} pieces")
    keep = pieces << log_n
    if out is None:
        out = torch.empty((max(keep, 1), 4), dtype=torch.int64, device=numer.device)
    elif (out.device != numer.device or out.dtype != torch.int64 or not out.is_contiguous() or out.dim() != 2
          or out.shape[1] != 4 or out.shape[0] < min(keep, N)):
        raise _lib.LengthError(f"quotient_coeffs: out must be a contiguous (>= {keep}, 4) int64 tensor on {numer.device}")
    gs = enc.fr_struct(shift, form) if shift is not None else None
    _lib.check(_lib.lib.sv_bn254_fr_quotient_coeffs_device(numer.data_ptr(), out.data_ptr(), log_n, K - log_n,
                                                           pieces,
                                                           ctypes.byref(gs) if gs is not None else None, form, d,
                                                           _stream_handle(numer.device)),
               "sv_bn254_fr_quotient_coeffs_device")
    return out[:keep]


# One factor of a grand product: kind (SV_FACTOR_*), x and -- COLUMN -- y as (n, 4) int64 tensors of
# limbs, s and c as canonical ints.  A plain tuple of the same fields, shorter where the rest is
# the default, does as well.
Factor = namedtuple("Factor", "kind x y s c", defaults=(None, 0, 0))


def _column(t: torch.Tensor, n: int, dev, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 4:
        raise _lib.ArgumentError(f"grand_product: {what} is an (n, 4) int64 tensor of limbs")
    if t.device != dev:
        raise _lib.ArgumentError("grand_product: the columns of a call live on one device")
    if t.shape[0] != n:
        raise _lib.LengthError(f"grand_product: {what} has {t.shape[0]} rows, the call {n}")
    return t.contiguous()


def factor_array(factors, form: int, n: int, dev, keep: list):
    """The host descriptor array (at least one element) of one side; the contiguous tensors it
    points into are appended to `keep`."""
    arr = (_lib.sv_fr_factor * max(len(factors), 1))()
    for j, f in enumerate(factors):
        f = Factor(*f)
        x = _column(f.x, n, dev, "x")
        keep.append(x)
        arr[j].d_x, arr[j].kind = x.data_ptr(), f.kind
        if f.kind == _lib.SV_FACTOR_COLUMN:
            y = _column(f.y, n, dev, "y")
            keep.append(y)
            arr[j].d_y = y.data_ptr()
        arr[j].s, arr[j].c = enc.fr_struct(f.s, form), enc.fr_struct(f.c, form)
    return arr


def grand_product_device(num, den, z0: int = 1, omega: Optional[int] = None, form: int = _lib.SV_MONTGOMERY,
                         out: torch.Tensor = None) -> Tuple[torch.Tensor, int]:
    """The running product z[0] = z0, z[i + 1] = z[i] prod_j num_j(i) / prod_j den_j(i) over HBM-resident
    columns ((n, 4) int64 limbs in `form`) -> (z as n rows in `form`, the total z0 prod_{i < n} as a
    canonical int).  num and den are lists of Factor (or tuples); z0, s, c and omega are canonical
    ints; omega = root_of_unity(k) is needed when a factor is SV_FACTOR_IDENTITY.  A row whose
    denominator is zero leaves every later z and the total zero.  `out` (n rows) must not overlap a
    column."""
    num, den = [Factor(*f) for f in num], [Factor(*f) for f in den]
    if not num and not den:
        raise _lib.EmptyError("grand_product: no factors")
    first = (num + den)[0].x
    d, dev, n = _dev_index(first), first.device, first.shape[0]
    keep: list = []
    na, da = factor_array(num, form, n, dev, keep), factor_array(den, form, n, dev, keep)
    if out is None:
        out = torch.empty((max(n, 1), 4), dtype=torch.int64, device=dev)
    elif (out.device != dev or out.dtype != torch.int64 or not out.is_contiguous() or out.dim() != 2
          or out.shape[1] != 4 or out.shape[0] != n):
        raise _lib.LengthError(f"grand_product: out must be a contiguous ({n}, 4) int64 tensor on {dev}")
    zs, total = enc.fr_struct(z0, form), _lib.sv_fe()
    ws = enc.fr_struct(omega, form) if omega is not None else None
    _lib.check(_lib.lib.sv_bn254_fr_grand_product_device(na, len(num), da, len(den), n, ctypes.byref(zs),
                                                         ctypes.byref(ws) if ws is not None else None, form,
                                                         out.data_ptr(), ctypes.byref(total), d, _stream_handle(dev)),
               "sv_bn254_fr_grand_product_device")
    return out[:n], enc.fr_from_struct(total, form)


def batch_invert_device(data: torch.Tensor, form: int = _lib.SV_MONTGOMERY, out: torch.Tensor = None) -> torch.Tensor:
    """1 / x for every row of an HBM-resident column ((n, 4) int64 limbs in `form`), 0 where x is 0.
    out=None allocates, out=data is in place; any other `out` (n rows) must not overlap data."""
    d = _dev_index(data)
    if data.dtype != torch.int64 or data.dim() != 2 or data.shape[1] != 4 or not data.is_contiguous():
        raise _lib.ArgumentError("batch_invert: data is a contiguous (n, 4) int64 tensor of limbs")
    if out is None:
        out = torch.empty_like(data)
    elif (out.device != data.device or out.dtype != torch.int64 or not out.is_contiguous()
          or out.shape != data.shape):
        raise _lib.LengthError(f"batch_invert: out must be a contiguous {tuple(data.shape)} int64 tensor on {data.device}")
    _lib.check(_lib.lib.sv_bn254_fr_batch_invert_device(data.data_ptr(), out.data_ptr(), data.shape[0], form, d,
                                                        _stream_handle(data.device)),
               "sv_bn254_fr_batch_invert_device")
    return out


def _fr_column(t: torch.Tensor, what: str) -> None:
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 4
            or not t.is_contiguous()):
        raise _lib.ArgumentError(f"{what} is a contiguous (n, 4) int64 tensor of limbs")


def sort_device(data: torch.Tensor, form: int = _lib.SV_MONTGOMERY, out: torch.Tensor = None) -> torch.Tensor:
    """An HBM-resident column ((n, 4) int64 limbs in `form`) sorted ascending by canonical value, in
    `form`.  out=None allocates, out=data is in place; any other `out` (n rows) must not overlap data."""
    d = _dev_index(data)
    _fr_column(data, "sort: data")
    if out is None:
        out = torch.empty_like(data)
    elif (out.device != data.device or out.dtype != torch.int64 or not out.is_contiguous()
          or out.shape != data.shape):
        raise _lib.LengthError(f"sort: out must be a contiguous {tuple(data.shape)} int64 tensor on {data.device}")
    _lib.check(_lib.lib.sv_bn254_fr_sort_device(data.data_ptr(), out.data_ptr(), data.shape[0], form, d,
                                                _stream_handle(data.device)),
               "sv_bn254_fr_sort_device")
    return out


def lookup_permute_device(inputs: torch.Tensor, tables: torch.Tensor, form: int = _lib.SV_MONTGOMERY,
                          out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """halo2's permute_expression_pair over HBM-resident columns ((n, 4) int64 limbs in `form`): the
    compressed input and table expressions of a lookup -> (permuted_input, permuted_table) in `form`.
    n is the usable rows; the blinding rows are the caller's.  out=None allocates; out=(a', s') are
    two n-row tensors that overlap neither each other nor an input.  An input value that is not in
    the table raises ArgumentError ("not in table") whose .row is the smallest such row of the
    permuted input."""
    d = _dev_index(inputs)
    _fr_column(inputs, "lookup_permute: inputs")
    _fr_column(tables, "lookup_permute: tables")
    if tables.device != inputs.device:
        raise _lib.ArgumentError("lookup_permute: the columns of a call live on one device")
    if tables.shape != inputs.shape:
        raise _lib.LengthError(f"lookup_permute: tables has {tables.shape[0]} rows, inputs {inputs.shape[0]}")
    if out is None:
        out = (torch.empty_like(inputs), torch.empty_like(inputs))
    for o in out:
        if (not isinstance(o, torch.Tensor) or o.device != inputs.device or o.dtype != torch.int64
                or not o.is_contiguous() or o.shape != inputs.shape):
            raise _lib.LengthError(f"lookup_permute: out is two contiguous {tuple(inputs.shape)} int64 tensors on "
                                   f"{inputs.device}")
    row = ctypes.c_uint64(0)
    rc = _lib.lib.sv_bn254_fr_lookup_permute_device(inputs.data_ptr(), tables.data_ptr(), inputs.shape[0], form,
                                                    out[0].data_ptr(), out[1].data_ptr(), ctypes.byref(row), d,
                                                    _stream_handle(inputs.device))
    try:
        _lib.check(rc, "sv_bn254_fr_lookup_permute_device")
    except _lib.ArgumentError as e:
        if "not in table" in str(e):
            e.row = row.value
        raise
    return out[0], out[1]


def lookup_permute_batch_device(inputs, tables, form: int = _lib.SV_MONTGOMERY, tables_sorted: bool = False, out=None):
    """lookup_permute_device for the lookups of a circuit in one call whose launch count does not
    depend on their number: `inputs` is a list of (n, 4) int64 tensors on one device, `tables` a list
    of the same length or one tensor that every lookup shares -> [(permuted_input, permuted_table),
    ..] in `form`, each pair what lookup_permute_device returns for that lookup.  Tables that are one
    tensor (the same data_ptr) are sorted once.  tables_sorted=True promises that every table is
    already ascending (what sort_device returns) and sorts none; a table that is not raises
    ArgumentError ("table not sorted").  out=None allocates; out=[(a', s'), ..] are n-row tensors that
    overlap nothing else of the call.  A value that is not in its table raises ArgumentError ("not in
    table") with .lookup = the first failing lookup and .rows = per lookup the smallest such row of
    its permuted input, None where the lookup is fine; the other lookups' outputs are then exact."""
    if isinstance(tables, torch.Tensor):
        tables = [tables] * len(inputs)
    inputs, tables = list(inputs), list(tables)
    if len(tables) != len(inputs):
        raise _lib.LengthError(f"lookup_permute_batch: {len(tables)} tables for {len(inputs)} inputs")
    if not inputs:
        raise _lib.EmptyError("lookup_permute_batch: the batch should not be empty")
    if len(inputs) > _lib.SV_LOOKUP_BATCH_MAX:
        raise _lib.LengthError(f"lookup_permute_batch: {len(inputs)} lookups exceed SV_LOOKUP_BATCH_MAX = "
                               f"{_lib.SV_LOOKUP_BATCH_MAX}")
    for j, (a, s) in enumerate(zip(inputs, tables)):
        _fr_column(a, f"lookup_permute_batch: inputs[{j}]")
        _fr_column(s, f"lookup_permute_batch: tables[{j}]")
    d = _dev_index(inputs[0])
    dev, shape = inputs[0].device, inputs[0].shape
    for t in inputs + tables:
        if t.device != dev:
            raise _lib.ArgumentError("lookup_permute_batch: the columns of a call live on one device")
        if t.shape != shape:
            raise _lib.LengthError(f"lookup_permute_batch: a column has {t.shape[0]} rows, inputs[0] {shape[0]}")
    if out is None:
        out = [(torch.empty_like(inputs[0]), torch.empty_like(inputs[0])) for _ in inputs]
    out = [tuple(pair) for pair in out]
    if len(out) != len(inputs) or any(len(pair) != 2 for pair in out):
        raise _lib.LengthError(f"lookup_permute_batch: out is {len(inputs)} pairs of tensors")
    for pair in out:
        for o in pair:
            if (not isinstance(o, torch.Tensor) or o.device != dev or o.dtype != torch.int64 or not o.is_contiguous()
                    or o.shape != shape):
                raise _lib.LengthError(f"lookup_permute_batch: out is pairs of contiguous {tuple(shape)} int64 tensors "
                                       f"on {dev}")
    count = len(inputs)
    ptrs = ctypes.c_void_p * count
    rows, failed = (ctypes.c_uint64 * count)(), ctypes.c_uint64(0)
    rc = _lib.lib.sv_bn254_fr_lookup_permute_batch_device(
        ptrs(*[t.data_ptr() for t in inputs]), ptrs(*[t.data_ptr() for t in tables]), count, shape[0], form,
        _lib.SV_LOOKUP_TABLES_SORTED if tables_sorted else 0, ptrs(*[p[0].data_ptr() for p in out]),
        ptrs(*[p[1].data_ptr() for p in out]), rows, ctypes.byref(failed), d, _stream_handle(dev))
    try:
        _lib.check(rc, "sv_bn254_fr_lookup_permute_batch_device")
    except _lib.ArgumentError as e:
        if "not in table" in str(e):
            e.lookup = failed.value
            e.rows = [None if r == 2**64 - 1 else r for r in rows]
        raise
    return out


def _terms_column(t: torch.Tensor, n: int, dev, who: str, what: str) -> torch.Tensor:
    """_column for the terms calls: an (N, 4) int64 tensor on the call's device, made contiguous."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 4:
        raise _lib.ArgumentError(f"{who}: {what} is an (N, 4) int64 tensor of limbs")
    if t.device != dev:
        raise _lib.ArgumentError(f"{who}: the columns of a call live on one device")
    if t.shape[0] != n:
        raise _lib.LengthError(f"{who}: {what} has {t.shape[0]} rows, the call {n}")
    return t.contiguous()


def _terms_shape(first: torch.Tensor, log_n: int, who: str) -> Tuple[int, int]:
    """(N, log_ext) of a terms call from its first column and the circuit's log_n."""
    if not isinstance(first, torch.Tensor) or first.dim() != 2:
        raise _lib.ArgumentError(f"{who}: a column is an (N, 4) int64 tensor of limbs")
    N = first.shape[0]
    if N == 0 or N & (N - 1):
        raise _lib.LengthError(f"{who}: {N} rows is not a power of two")
    K = N.bit_length() - 1
    if not 0 <= log_n <= K:
        raise _lib.LengthError(f"{who}: log_n = {log_n} is not in 0 .. {K}")
    return N, K - log_n


def _terms_out(out, acc, N: int, dev, who: str):
    """The accumulator (or None) and the output of a terms call; out=None allocates, out=acc is in place."""
    if acc is not None:
        acc = _terms_column(acc, N, dev, who, "acc")
    if out is None:
        out = torch.empty((N, 4), dtype=torch.int64, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.int64
          or not out.is_contiguous() or tuple(out.shape) != (N, 4)):
        raise _lib.LengthError(f"{who}: out must be a contiguous ({N}, 4) int64 tensor on {dev}")
    return acc, out


def _pointer_array(tensors):
    arr = (ctypes.c_void_p * max(len(tensors), 1))()
    for j, t in enumerate(tensors):
        arr[j] = t.data_ptr()
    return arr


def permutation_terms_device(cols, sigmas, s, chunk: int, z, l0: torch.Tensor, l_last: torch.Tensor,
                             l_active: torch.Tensor, beta: int, gamma: int, y: int, log_n: int,
                             last_rotation: int, shift: Optional[int] = None, acc: torch.Tensor = None,
                             form: int = _lib.SV_MONTGOMERY, out: torch.Tensor = None) -> torch.Tensor:
    """The permutation argument's constraints (system/halo2.rs:501-591) on HBM-resident extended
    columns ((N, 4) int64 limbs in `form`, N = 2^(log_n + log_ext), row j at shift omega_K^j), folded in
    y onto `acc` (None = 0): per constraint c, acc <- acc y + c.  cols and sigmas are the m permutation
    columns and their sigmas, s the m canonical ints beta delta^j, z the ceil(m / chunk) running
    products; l0, l_last, l_active the selector columns; last_rotation = -(blinding + 1).  beta,
    gamma, y and shift (None = 1) are canonical ints.  out=None allocates, out=acc is in place; any
    other `out` (N rows) must not overlap an input."""
    who = "permutation_terms"
    cols, sigmas, z, s = list(cols), list(sigmas), list(z), list(s)
    if not cols:
        raise _lib.EmptyError(f"{who}: no permutation columns")
    if chunk < 1:
        raise _lib.ArgumentError(f"{who}: chunk = {chunk}: a z column covers at least one permutation column")
    if not len(cols) == len(sigmas) == len(s):
        raise _lib.LengthError(f"{who}: cols, sigmas and s differ in length")
    m = len(cols)
    if len(z) != -(-m // chunk):
        raise _lib.LengthError(f"{who}: {len(z)} z columns, {m} columns in chunks of {chunk} need {-(-m // chunk)}")
    N, log_ext = _terms_shape(cols[0], log_n, who)
    d, dev = _dev_index(cols[0]), cols[0].device
    cols = [_terms_column(t, N, dev, who, "a column") for t in cols]
    sigmas = [_terms_column(t, N, dev, who, "a sigma") for t in sigmas]
    z = [_terms_column(t, N, dev, who, "a z") for t in z]
    l0, l_last, l_active = (_terms_column(t, N, dev, who, "an l column") for t in (l0, l_last, l_active))
    acc, out = _terms_out(out, acc, N, dev, who)
    bs, gs, ys = enc.fr_struct(beta, form), enc.fr_struct(gamma, form), enc.fr_struct(y, form)
    sh = enc.fr_struct(shift, form) if shift is not None else None
    _lib.check(_lib.lib.sv_bn254_fr_permutation_terms_device(
        _pointer_array(cols), _pointer_array(sigmas), fe_array(s, form), m, chunk, _pointer_array(z),
        l0.data_ptr(), l_last.data_ptr(), l_active.data_ptr(), ctypes.byref(bs), ctypes.byref(gs), ctypes.byref(ys),
        ctypes.byref(sh) if sh is not None else None, last_rotation, acc.data_ptr() if acc is not None else None,
        out.data_ptr(), log_n, log_ext, form, d, _stream_handle(dev)), "sv_bn254_fr_permutation_terms_device")
    return out


def lookup_terms_device(lookups, l0: torch.Tensor, l_last: torch.Tensor, l_active: torch.Tensor, beta: int,
                        gamma: int, y: int, log_n: int, acc: torch.Tensor = None, form: int = _lib.SV_MONTGOMERY,
                        out: torch.Tensor = None) -> torch.Tensor:
    """Each lookup's five constraints (system/halo2.rs:593-655) on HBM-resident extended columns ((N,
    4) int64 limbs in `form`), folded in y onto `acc` (None = 0).  lookups is a list of (z,
    permuted_input, permuted_table, input, table); l0, l_last, l_active the selector columns; beta,
    gamma, y canonical ints.  out=None allocates, out=acc is in place; any other `out` (N rows) must
    not overlap an input."""
    who = "lookup_terms"
    lookups = [tuple(lk) for lk in lookups]
    if not lookups:
        raise _lib.EmptyError(f"{who}: no lookups")
    if any(len(lk) != 5 for lk in lookups):
        raise _lib.ArgumentError(f"{who}: a lookup is (z, permuted_input, permuted_table, input, table)")
    first = lookups[0][0]
    N, log_ext = _terms_shape(first, log_n, who)
    d, dev = _dev_index(first), first.device
    lookups = [tuple(_terms_column(t, N, dev, who, "a lookup column") for t in lk) for lk in lookups]
    l0, l_last, l_active = (_terms_column(t, N, dev, who, "an l column") for t in (l0, l_last, l_active))
    acc, out = _terms_out(out, acc, N, dev, who)
    arr = (_lib.sv_fr_lookup * len(lookups))()
    for j, lk in enumerate(lookups):
        (arr[j].d_z, arr[j].d_permuted_input, arr[j].d_permuted_table, arr[j].d_input,
         arr[j].d_table) = (t.data_ptr() for t in lk)
    bs, gs, ys = enc.fr_struct(beta, form), enc.fr_struct(gamma, form), enc.fr_struct(y, form)
    _lib.check(_lib.lib.sv_bn254_fr_lookup_terms_device(
        arr, len(lookups), l0.data_ptr(), l_last.data_ptr(), l_active.data_ptr(), ctypes.byref(bs), ctypes.byref(gs),
        ctypes.byref(ys), acc.data_ptr() if acc is not None else None, out.data_ptr(), log_n, log_ext, form, d,
        _stream_handle(dev)), "sv_bn254_fr_lookup_terms_device")
    return out


def expressions_device(program, cols, consts, stores=(), y: Optional[int] = None, acc: torch.Tensor = None,
                       out: torch.Tensor = None, log_n: int = None, form: int = _lib.SV_MONTGOMERY):
    """A postfix expression program (include/svgpu.h; svgpu.compile_expressions makes one from
    trees) at every row of HBM-resident columns ((N, 4) int64 limbs in `form`, N = 2^(log_n +
    log_ext)): custom gates folded in y onto `acc` (None = 0), per FOLD acc <- acc y + v, and columns
    written by STORE.  program is a list of (op, index, rotation); cols the columns it names by index;
    consts and y canonical ints; stores the tensors STORE k writes, or an int to allocate that many.
    out=None allocates when the program folds, out=acc is in place.  Returns (out, stores): out is
    None for a program without a FOLD."""
    who = "expressions"
    program, cols, consts = [tuple(o) for o in program], list(cols), list(consts)
    if log_n is None:
        raise _lib.ArgumentError(f"{who}: log_n is required")
    if any(len(o) != 3 for o in program):
        raise _lib.ArgumentError(f"{who}: an op is (op, index, rotation)")
    first = cols[0] if cols else (stores[0] if not isinstance(stores, int) and len(stores) else acc)
    if first is None:
        raise _lib.ArgumentError(f"{who}: no column, store or acc tells the number of rows")
    N, log_ext = _terms_shape(first, log_n, who)
    d, dev = _dev_index(first), first.device
    cols = [_terms_column(t, N, dev, who, "a column") for t in cols]
    if isinstance(stores, int):
        stores = [torch.empty((N, 4), dtype=torch.int64, device=dev) for _ in range(stores)]
    stores = list(stores)
    for t in stores:
        if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.int64 or not t.is_contiguous()
                or tuple(t.shape) != (N, 4)):
            raise _lib.LengthError(f"{who}: a store must be a contiguous ({N}, 4) int64 tensor on {dev}")
    folds = any(o[0] == _lib.SV_EXPR_FOLD for o in program)
    if folds:
        if y is None:
            raise _lib.ArgumentError(f"{who}: a program that folds needs y")
        acc, out = _terms_out(out, acc, N, dev, who)
    else:
        acc = out = None
    ops = (_lib.sv_fr_expr_op * max(len(program), 1))()
    for i, (op, index, rotation) in enumerate(program):
        if not (0 <= op < 256 and 0 <= index < 65536 and -(1 << 31) <= rotation < (1 << 31)):
            raise _lib.ArgumentError(f"{who}: op {i} = ({op}, {index}, {rotation}) does not fit an op")
        ops[i].op, ops[i].index, ops[i].rotation = op, index, rotation
    ys = enc.fr_struct(y, form) if y is not None else None
    _lib.check(_lib.lib.sv_bn254_fr_expressions_device(
        ops, len(program), _pointer_array(cols), len(cols), fe_array(consts, form) if consts else None, len(consts),
        _pointer_array(stores), len(stores), ctypes.byref(ys) if ys is not None else None,
        acc.data_ptr() if acc is not None else None, out.data_ptr() if out is not None else None, log_n, log_ext,
        form, d, _stream_handle(dev)), "sv_bn254_fr_expressions_device")
    return out, stores


def lagrange_selectors_device(k: int, log_ext: int, blinding: int, shift: Optional[int] = None,
                              form: int = _lib.SV_MONTGOMERY, device=None):
    """The selector columns of the zk quotient on the extended domain, (l0, l_last, l_active,
    last_rotation): with n = 2^k and u = n - blinding - 1 the last usable row, l0 is the Lagrange
    polynomial of row 0, l_last that of row u, l_active the indicator of rows [0, u), each as (2^(k +
    log_ext), 4) limbs in `form` at shift omega_K^j; last_rotation = -(blinding + 1).  Built from the
    three indicator columns through ntt_device(inverse=True) and coset_lde_device with count 3."""
    n = 1 << k
    if blinding < 0 or blinding + 1 >= n:
        raise _lib.LengthError(f"lagrange_selectors: blinding = {blinding} leaves no usable row of {n}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    u = n - blinding - 1
    one = np.asarray(enc.scalars_array([1], form)).view(np.int64).reshape(4)
    ind = np.zeros((3, n, 4), np.int64)
    ind[0, 0] = one
    ind[1, u] = one
    ind[2, :u] = one
    coeffs = ntt_device(torch.from_numpy(ind).to(dev), inverse=True, form=form)
    ext = coset_lde_device(coeffs, log_ext, shift=shift, form=form)
    return ext[0], ext[1], ext[2], -(blinding + 1)


def last_msm_stats() -> dict:
    s = _lib.sv_msm_stats()
    _lib.check(_lib.lib.sv_msm_last_stats(ctypes.byref(s)), "sv_msm_last_stats")
    return {name: getattr(s, name) for name, _ in s._fields_}


def decide(g2, s_g2, lhs: torch.Tensor, rhs: torch.Tensor, form: int = _lib.SV_CANONICAL,
           want_gt: bool = False) -> Tuple[int, List[int], Optional[List[List[int]]]]:
    """Decider over HBM-resident accumulators -> (first_fail, verdicts, Gt values or None)."""
    n = lhs.shape[0]
    d = _dev_index(lhs)
    ff = ctypes.c_int32(-2)
    # numpy buffer + tolist(): 256 verdicts in ~5 us where list() of a ctypes array took ~15 us
    verdicts = np.empty(n, dtype=np.int32)
    gt = (_lib.sv_fq12 * n)() if want_gt else None
    g2s, sg2s = _g2_struct_cached(g2, form), _g2_struct_cached(s_g2, form)
    _lib.check(_lib.lib.sv_bn254_kzg_decide_device(
        ctypes.byref(g2s), ctypes.byref(sg2s), lhs.data_ptr(), rhs.data_ptr(), n, form, d,
        _stream_handle(lhs.device), ctypes.byref(ff), verdicts.ctypes.data,
        ctypes.cast(gt, ctypes.c_void_p) if gt is not None else None), "sv_bn254_kzg_decide_device")
    gts = [enc.fq12_from_struct(g) for g in gt] if gt is not None else None
    return ff.value, verdicts.tolist(), gts


_G2_CACHE: dict = {}
# The same key object passed again (the usual verifier loop): (id, form) -> (object, a deep copy of
# it, struct).  A hit needs the very object AND equal contents (a C-level compare, ~0.1 us), so a
# list mutated in place misses; the content-keyed _G2_CACHE below costs ~2.7 us (Python freezing).
_G2_RECENT: dict = {}


def _frozen(v):
    """Nested lists (a G2 point as ((x0, x1), (y0, y1)) in any sequence type) as nested tuples."""
    return tuple(_frozen(x) for x in v) if isinstance(v, (list, tuple)) else v


def _g2_struct_cached(q, form: int):
    """A deciding key's G2 point as its ABI struct, converted once per key (a verifier decides with
    one key over and over; the library only reads the struct during the call)."""
    plain = type(q) in (list, tuple)
    if plain:
        e = _G2_RECENT.get((id(q), form))
        try:
            if e is not None and e[0] is q and bool(e[1] == q):
                return e[2]
        except (TypeError, ValueError):  # elements whose == is not a plain bool (arrays): no fast path
            plain = False
    try:
        key = (_frozen(q), form)
        hash(key)
    except TypeError:  # something hash cannot take even after freezing: no caching
        return enc.g2_struct(q, form)
    s = _G2_CACHE.get(key)
    if s is None:
        if len(_G2_CACHE) >= 16:
            _G2_CACHE.clear()
        s = _G2_CACHE[key] = enc.g2_struct(q, form)
    if plain:
        if len(_G2_RECENT) >= 16:
            _G2_RECENT.clear()
        _G2_RECENT[(id(q), form)] = (q, copy.deepcopy(q), s)
    return s


def last_decide_kernel_ms() -> float:
    """Kernel time of this thread's last decider launch (HIP events on the call's stream)."""
    v = ctypes.c_float(0)
    _lib.check(_lib.lib.sv_kzg_last_kernel_ms(ctypes.byref(v)), "sv_kzg_last_kernel_ms")
    return float(v.value)


def poseidon_squeeze(states: torch.Tensor, elements: torch.Tensor, offsets: torch.Tensor, t: int = 3,
                     form: int = _lib.SV_MONTGOMERY, out: torch.Tensor = None) -> torch.Tensor:
    """Poseidon::squeeze on n HBM-resident sponges (states: (n * t, 4) int64 limbs, in/out;
    elements: (m, 4); offsets: (n + 1,) int64, sponge j absorbs elements[offsets[j]:offsets[j+1]]).
    Returns out (n, 4): the challenges."""
    n = offsets.shape[0] - 1
    if states.shape[0] != n * t:
        raise _lib.LengthError(f"poseidon: {states.shape[0]} state rows for {n} sponges of width {t}")
    if out is None:
        out = torch.empty((max(n, 1), 4), dtype=torch.int64, device=states.device)
    d = _dev_index(states)
    _lib.check(_lib.lib.sv_bn254_poseidon_squeeze_device(states.data_ptr(), elements.data_ptr(), offsets.data_ptr(),
                                                         n, t, form, out.data_ptr(), d,
                                                         _stream_handle(states.device)),
               "sv_bn254_poseidon_squeeze_device")
    return out[:n]


def poseidon_permute(states: torch.Tensor, t: int = 3, form: int = _lib.SV_MONTGOMERY) -> torch.Tensor:
    """In-place HADES permutation of (n * t, 4) HBM-resident states."""
    d = _dev_index(states)
    _lib.check(_lib.lib.sv_bn254_poseidon_permute_device(states.data_ptr(), states.shape[0] // t, t, form, d,
                                                         _stream_handle(states.device)),
               "sv_bn254_poseidon_permute_device")
    return states


def msm_batch(bases: torch.Tensor, scalars: torch.Tensor, offsets: torch.Tensor, max_terms: int,
              form: int = _lib.SV_MONTGOMERY, out: torch.Tensor = None) -> torch.Tensor:
    """Batched MSMs over HBM-resident arrays (offsets: (count + 1,) int64 on the device);
    returns (count, 8) int64 affine results in `form`."""
    count = offsets.shape[0] - 1
    if out is None:
        out = torch.empty((max(count, 1), 8), dtype=torch.int64, device=bases.device)
    d = _dev_index(bases)
    _lib.check(_lib.lib.sv_bn254_g1_msm_batch_device(bases.data_ptr(), scalars.data_ptr(), offsets.data_ptr(),
                                                     count, max_terms, form, d, _stream_handle(bases.device),
                                                     out.data_ptr()),
               "sv_bn254_g1_msm_batch_device")
    return out[:count]


def msm_batch_indexed(table: torch.Tensor, base_idx: torch.Tensor, scalars: torch.Tensor, offsets: torch.Tensor,
                      max_terms: int, form: int = _lib.SV_MONTGOMERY, table_form: int = _lib.SV_MONTGOMERY,
                      out: torch.Tensor = None) -> torch.Tensor:
    """Batched MSMs whose terms reference rows of an HBM-resident base table (table: (rows, 8) int64;
    base_idx: (terms,) int32 row indices; offsets: (count + 1,) int64); returns (count, 8) int64."""
    count = offsets.shape[0] - 1
    if out is None:
        out = torch.empty((max(count, 1), 8), dtype=torch.int64, device=scalars.device)
    d = _dev_index(scalars)
    _lib.check(_lib.lib.sv_bn254_g1_msm_batch_indexed_device(table.data_ptr(), table.shape[0], table_form,
                                                             base_idx.data_ptr(), scalars.data_ptr(),
                                                             offsets.data_ptr(), count, max_terms, form, d,
                                                             _stream_handle(scalars.device), out.data_ptr()),
               "sv_bn254_g1_msm_batch_indexed_device")
    return out[:count]
