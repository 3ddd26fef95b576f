"""Host-side mirror of the reference's MSM entry points, executed by libsvgpu on the GPU.

* ``NativeLoader.multi_scalar_multiplication(pairs)`` mirrors
  ``EcPointLoader::multi_scalar_multiplication`` for ``NativeLoader``
  (snark-verifier/src/loader/native.rs:61-71): sum of ``base * scalar`` over the pairs, as an
  affine point; empty input panics with "pairs should not be empty" (native.rs:69).
* ``multi_scalar_multiplication(scalars, bases)`` mirrors ``util::msm::multi_scalar_multiplication``
  (snark-verifier/src/util/msm.rs:287-316), whose length check is ``assert_eq!`` (msm.rs:288).

* ``batch_multi_scalar_multiplication(msms)`` / ``NativeLoader.multi_scalar_multiplication_batch``
  evaluate many such MSMs in one call (the per-proof Msm::evaluate calls of a
  native verifier, bdfg21.rs:75-78 / gwc19.rs:76-79, and accumulation.rs:177-192's pair).

Points are ``(x, y)`` tuples of canonical ints, ``None`` is the identity (halo2curves (0, 0)).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import encoding as enc

Point = Optional[Tuple[int, int]]


class ReferencePanic(AssertionError):
    """A condition under which the Rust reference panics."""


def msm_arrays(bases: np.ndarray, scalars: np.ndarray, form: int = _lib.SV_CANONICAL, num_gpus: int = 0) -> Point:
    """MSM over C-ABI-layout host arrays: bases (n, 8) u64, scalars (n, 4) u64."""
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    if bases.shape[0] != scalars.shape[0]:
        raise ReferencePanic("assertion failed: scalars.len() == bases.len()")
    out = _lib.sv_g1_affine()
    rc = _lib.lib.sv_bn254_g1_msm(bases.ctypes.data, scalars.ctypes.data, bases.shape[0], form, num_gpus,
                                  ctypes.byref(out))
    if rc == _lib.SV_ERR_EMPTY:
        raise ReferencePanic("pairs should not be empty")
    _lib.check(rc, "sv_bn254_g1_msm")
    return enc.g1_from_struct(out, form)


def make_refs(scalar_ptrs: np.ndarray, base_ptrs: np.ndarray) -> np.ndarray:
    """Pack two equal-length arrays of host addresses (scalar_ptrs[i] -> sv_fe, base_ptrs[i] ->
    sv_g1_affine) into the (n, 2) u64 sv_msm_ref array of the C ABI."""
    sp = np.ascontiguousarray(scalar_ptrs, dtype=np.uint64)
    bp = np.ascontiguousarray(base_ptrs, dtype=np.uint64)
    if sp.shape != bp.shape:
        raise ReferencePanic("assertion failed: scalars.len() == bases.len()")
    return np.stack([sp, bp], axis=1)


def msm_refs(refs: np.ndarray, form: int = _lib.SV_CANONICAL, num_gpus: int = 0) -> Point:
    """MSM over references (the NativeLoader pairs shape, native.rs:61-71): `refs` is the (n, 2)
    u64 sv_msm_ref array (see make_refs); the library gathers the referenced values."""
    refs = np.ascontiguousarray(refs, dtype=np.uint64).reshape(-1, 2)
    out = _lib.sv_g1_affine()
    rc = _lib.lib.sv_bn254_g1_msm_refs(refs.ctypes.data, refs.shape[0], form, num_gpus, ctypes.byref(out))
    if rc == _lib.SV_ERR_EMPTY:
        raise ReferencePanic("pairs should not be empty")
    _lib.check(rc, "sv_bn254_g1_msm_refs")
    return enc.g1_from_struct(out, form)


def multi_scalar_multiplication(scalars: Sequence[int], bases: Sequence[Point], num_gpus: int = 0) -> Point:
    if len(scalars) != len(bases):
        raise ReferencePanic("assertion failed: scalars.len() == bases.len()")
    return msm_arrays(enc.bases_array(bases), enc.scalars_array(scalars), _lib.SV_CANONICAL, num_gpus)


def msm_batch_arrays(bases: np.ndarray, scalars: np.ndarray, offsets: Sequence[int],
                     form: int = _lib.SV_CANONICAL) -> list:
    """len(offsets) - 1 MSMs over shared C-ABI host arrays; MSM k uses rows offsets[k]:offsets[k+1]."""
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    if bases.shape[0] != scalars.shape[0]:
        raise ReferencePanic("assertion failed: scalars.len() == bases.len()")
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    count = off.shape[0] - 1
    if count <= 0:
        return []
    if int(off[-1]) > bases.shape[0]:
        raise _lib.LengthError("msm_batch: offsets run past the arrays")
    out = (_lib.sv_g1_affine * count)()
    rc = _lib.lib.sv_bn254_g1_msm_batch(bases.ctypes.data, scalars.ctypes.data, off.ctypes.data, count, form,
                                        ctypes.cast(out, ctypes.c_void_p))
    if rc == _lib.SV_ERR_EMPTY:
        raise ReferencePanic("pairs should not be empty")
    _lib.check(rc, "sv_bn254_g1_msm_batch")
    return [enc.g1_from_struct(o, form) for o in out]


class BaseTable:
    """Device-resident fixed bases (the generator and a circuit's preprocessed commitments, loaded
    once per verifier: Protocol::loaded, plonk/protocol.rs:106-131) referenced by row index from
    each proof's MSMs (Msm::evaluate, bdfg21.rs:75-78 / gwc19.rs:76-79), so a per-proof batch ships
    only scalars and u32 indices.  Rows are uploaded once in Montgomery form on `device` and expanded
    there to their window multiples 2^(8 w) P, so every batch runs in one bucket set per MSM with
    no window Horner (csrc/msm_batch.hip k_msm_batch_fixed)."""

    def __init__(self, bases, device: int = 0):
        if not isinstance(bases, np.ndarray):
            bases = enc.bases_array(list(bases))
        arr = np.ascontiguousarray(bases, dtype=np.uint64)
        self.n = arr.shape[0]
        self.handle = None
        h = ctypes.c_uint64(0)
        _lib.check(_lib.lib.sv_bn254_g1_table_create(arr.ctypes.data, self.n, _lib.SV_CANONICAL, device,
                                                     ctypes.byref(h)), "sv_bn254_g1_table_create")
        self.handle = h.value

    def close(self):
        if self.handle is not None:
            h, self.handle = self.handle, None
            _lib.check(_lib.lib.sv_bn254_g1_table_destroy(h), "sv_bn254_g1_table_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def msm_batch_arrays(self, base_idx: np.ndarray, scalars: np.ndarray, offsets: Sequence[int],
                         form: int = _lib.SV_CANONICAL) -> list:
        """MSM k = sum over i in [offsets[k], offsets[k+1]) of scalars[i] * table[base_idx[i]]."""
        if self.handle is None:
            raise _lib.ArgumentError("base table is closed")
        idx = np.ascontiguousarray(base_idx, dtype=np.uint32)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        if idx.shape[0] != scalars.shape[0]:
            raise ReferencePanic("assertion failed: scalars.len() == bases.len()")
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        count = off.shape[0] - 1
        if count <= 0:
            return []
        if int(off[-1]) > idx.shape[0]:
            raise _lib.LengthError("msm_batch: offsets run past the arrays")
        out = (_lib.sv_g1_affine * count)()
        rc = _lib.lib.sv_bn254_g1_msm_batch_table(self.handle, idx.ctypes.data, scalars.ctypes.data,
                                                  off.ctypes.data, count, form, ctypes.cast(out, ctypes.c_void_p))
        if rc == _lib.SV_ERR_EMPTY:
            raise ReferencePanic("pairs should not be empty")
        _lib.check(rc, "sv_bn254_g1_msm_batch_table")
        return [enc.g1_from_struct(o, form) for o in out]

    def device(self) -> int:
        d = ctypes.c_int(-1)
        _lib.check(_lib.lib.sv_bn254_g1_table_device(self.handle, ctypes.byref(d)), "sv_bn254_g1_table_device")
        return d.value

    def msm_batch_device(self, base_idx, scalars, offsets, form: int = _lib.SV_MONTGOMERY, out=None):
        """HBM-resident form (torch tensors on the table's device): base_idx (terms,) int32, scalars
        (terms, 4) int64, offsets (count + 1,) int64 -> (count, 8) int64 affine results in `form`."""
        import torch
        if self.handle is None:
            raise _lib.ArgumentError("base table is closed")
        count = offsets.shape[0] - 1
        if out is None:
            out = torch.empty((max(count, 1), 8), dtype=torch.int64, device=scalars.device)
        stream = torch.cuda.current_stream(scalars.device).cuda_stream
        _lib.check(_lib.lib.sv_bn254_g1_msm_batch_table_device(self.handle, base_idx.data_ptr(), scalars.data_ptr(),
                                                                offsets.data_ptr(), count, form, stream,
                                                                out.data_ptr()), "sv_bn254_g1_msm_batch_table_device")
        return out[:count]

    def batch_multi_scalar_multiplication(self, msms: Sequence[Sequence[Tuple[int, int]]]) -> list:
        """msms: per MSM a list of (scalar, table row) pairs."""
        offsets = [0]
        scalars, idx = [], []
        for pairs in msms:
            if len(pairs) == 0:
                raise ReferencePanic("pairs should not be empty")
            scalars += [s for s, _ in pairs]
            idx += [i for _, i in pairs]
            offsets.append(len(scalars))
        if not msms:
            return []
        return self.msm_batch_arrays(np.array(idx, dtype=np.uint32), enc.scalars_array(scalars), offsets)


class ResidentBases:
    """A resident base set for large MSMs: the bases of a KZG MSM (the SRS, a Lagrange basis, a
    committing key) uploaded ONCE to `device` and kept there in the form the MSM pipeline consumes
    (208 B per point: Montgomery rows + the accumulate's 29-bit table of P and phi(P)), so each MSM
    ships only its scalars and prepares no base.  `bases`: an (n, 8) u64 array in `form`, or a
    sequence of points.  One set lives on one device; with several GPUs make one set per device
    over its shard and fold the partials (fold_partials)."""

    def __init__(self, bases, device: int = 0, form: int = _lib.SV_CANONICAL):
        self.handle = None
        if not isinstance(bases, np.ndarray):
            bases = enc.bases_array(list(bases))
        arr = np.ascontiguousarray(bases, dtype=np.uint64)
        h = ctypes.c_uint64(0)
        _lib.check(_lib.lib.sv_bn254_g1_bases_create(arr.ctypes.data, arr.shape[0], form, device, ctypes.byref(h)),
                   "sv_bn254_g1_bases_create")
        self.handle = h.value
        self._info()

    @classmethod
    def from_device(cls, tensor, form: int = _lib.SV_MONTGOMERY) -> "ResidentBases":
        """A set over rows already in HBM: an (n, 8) int64 torch tensor in `form`; the set lives on the
        tensor's device and keeps its own copy (the tensor may be freed afterwards)."""
        import torch
        if tensor.device.type != "cuda":
            raise _lib.DeviceError("tensor must live on a GPU (cuda/HIP device)")
        tensor = tensor.contiguous()
        d = tensor.device.index if tensor.device.index is not None else torch.cuda.current_device()
        self = cls.__new__(cls)
        self.handle = None
        h = ctypes.c_uint64(0)
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
        _lib.check(_lib.lib.sv_bn254_g1_bases_create_device(tensor.data_ptr(), tensor.shape[0], form, d, stream,
                                                            ctypes.byref(h)), "sv_bn254_g1_bases_create_device")
        self.handle = h.value
        self._info()
        return self

    def _info(self):
        n, d, b = ctypes.c_uint64(0), ctypes.c_int(-1), ctypes.c_uint64(0)
        _lib.check(_lib.lib.sv_bn254_g1_bases_info(self.handle, ctypes.byref(n), ctypes.byref(d), ctypes.byref(b)),
                   "sv_bn254_g1_bases_info")
        self.n, self.device, self.device_bytes = n.value, d.value, b.value

    def close(self):
        if self.handle is not None:
            h, self.handle = self.handle, None
            _lib.check(_lib.lib.sv_bn254_g1_bases_destroy(h), "sv_bn254_g1_bases_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def msm_arrays(self, scalars: np.ndarray, offset: int = 0, form: int = _lib.SV_CANONICAL) -> Point:
        """sum_i scalars[i] * set[offset + i] over host scalars ((n, 4) u64 in `form`)."""
        if self.handle is None:
            raise _lib.ArgumentError("base set is closed")
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        out = _lib.sv_g1_affine()
        rc = _lib.lib.sv_bn254_g1_msm_bases(self.handle, offset, scalars.ctypes.data, scalars.shape[0], form,
                                            ctypes.byref(out))
        if rc == _lib.SV_ERR_EMPTY:
            raise ReferencePanic("pairs should not be empty")
        _lib.check(rc, "sv_bn254_g1_msm_bases")
        return enc.g1_from_struct(out, form)

    def _partial_struct(self, scalars, offset: int, form: int):
        import torch
        if self.handle is None:
            raise _lib.ArgumentError("base set is closed")
        if scalars.device.type != "cuda":
            raise _lib.DeviceError("tensor must live on a GPU (cuda/HIP device)")
        part = _lib.sv_g1_jacobian()
        stream = torch.cuda.current_stream(scalars.device).cuda_stream
        rc = _lib.lib.sv_bn254_g1_msm_bases_device(self.handle, offset, scalars.data_ptr(), scalars.shape[0], form,
                                                   stream, ctypes.byref(part))
        if rc == _lib.SV_ERR_EMPTY:
            raise ReferencePanic("pairs should not be empty")
        _lib.check(rc, "sv_bn254_g1_msm_bases_device")
        return part

    def msm_device_partial(self, scalars, offset: int = 0, form: int = _lib.SV_MONTGOMERY) -> Tuple[int, int, int]:
        """sum_i scalars[i] * set[offset + i] over scalars in HBM on the set's device ((n, 4) int64
        torch tensor in `form`) -> canonical Jacobian partial (X, Y, Z), the value to fold across
        devices (fold_partials)."""
        return enc.jacobian_from_struct(self._partial_struct(scalars, offset, form))

    def msm_device(self, scalars, offset: int = 0, form: int = _lib.SV_MONTGOMERY) -> Point:
        """The same as an affine point (canonical ints; None = identity): the partial goes straight
        into sv_bn254_g1_fold."""
        part = self._partial_struct(scalars, offset, form)
        out = _lib.sv_g1_affine()
        _lib.check(_lib.lib.sv_bn254_g1_fold(ctypes.byref(part), 1, ctypes.byref(out), _lib.SV_CANONICAL),
                   "sv_bn254_g1_fold")
        return enc.g1_from_struct(out)


    def open_arrays(self, coeffs: np.ndarray, z: int, offset: int = 0,
                    form: int = _lib.SV_CANONICAL) -> Tuple[int, Point]:
        """KZG opening of p(X) = sum_i coeffs[i] X^i at z over set[offset:]: host coefficients
        ((n, 4) u64 in `form`), z a canonical int -> (p(z), witness), both canonical
        (sv_bn254_kzg_open: the division and the witness MSM run on the device)."""
        if self.handle is None:
            raise _lib.ArgumentError("base set is closed")
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
        zs, ev, out = enc.fr_struct(z, form), _lib.sv_fe(), _lib.sv_g1_affine()
        _lib.check(_lib.lib.sv_bn254_kzg_open(self.handle, offset, coeffs.ctypes.data, coeffs.shape[0],
                                              ctypes.byref(zs), form, ctypes.byref(ev), ctypes.byref(out)),
                   "sv_bn254_kzg_open")
        return enc.fr_from_struct(ev, form), enc.g1_from_struct(out, form)

    def open_device(self, coeffs, z: int, offset: int = 0, form: int = _lib.SV_MONTGOMERY) -> Tuple[int, Point]:
        """The same for coefficients in HBM on the set's device ((n, 4) int64 torch tensor in `form`):
        they never leave the device (sv_bn254_kzg_open_device; the partial is folded on the host)."""
        import torch
        if self.handle is None:
            raise _lib.ArgumentError("base set is closed")
        if coeffs.device.type != "cuda":
            raise _lib.DeviceError("tensor must live on a GPU (cuda/HIP device)")
        coeffs = coeffs.contiguous()
        zs, ev, part = enc.fr_struct(z, form), _lib.sv_fe(), _lib.sv_g1_jacobian()
        stream = torch.cuda.current_stream(coeffs.device).cuda_stream
        _lib.check(_lib.lib.sv_bn254_kzg_open_device(self.handle, offset, coeffs.data_ptr(), coeffs.shape[0],
                                                     ctypes.byref(zs), form, stream, ctypes.byref(ev),
                                                     ctypes.byref(part)), "sv_bn254_kzg_open_device")
        out = _lib.sv_g1_affine()
        _lib.check(_lib.lib.sv_bn254_g1_fold(ctypes.byref(part), 1, ctypes.byref(out), _lib.SV_CANONICAL),
                   "sv_bn254_g1_fold")
        return enc.fr_from_struct(ev, form), enc.g1_from_struct(out)

    def open_batch_pointers(self, ptrs, lens, m: int, z: int, v: int, offset: int, form: int,
                            stream) -> Tuple[list, Point]:
        """sv_bn254_kzg_open_batch_device over raw host arrays of m device pointers and lengths (what
        open_batch_device builds from tensors) -> ([p_j(z)], witness), canonical."""
        if self.handle is None:
            raise _lib.ArgumentError("base set is closed")
        zs, vs = enc.fr_struct(z, form), enc.fr_struct(v, form)
        ev, part = (_lib.sv_fe * max(m, 1))(), _lib.sv_g1_jacobian()
        _lib.check(_lib.lib.sv_bn254_kzg_open_batch_device(self.handle, offset, ptrs, lens, m, ctypes.byref(zs),
                                                           ctypes.byref(vs), form, stream, ev, ctypes.byref(part)),
                   "sv_bn254_kzg_open_batch_device")
        out = _lib.sv_g1_affine()
        _lib.check(_lib.lib.sv_bn254_g1_fold(ctypes.byref(part), 1, ctypes.byref(out), _lib.SV_CANONICAL),
                   "sv_bn254_g1_fold")
        return [enc.fr_from_struct(ev[j], form) for j in range(m)], enc.g1_from_struct(out)

    def open_batch_device(self, polys, z: int, v: int, offset: int = 0,
                          form: int = _lib.SV_MONTGOMERY) -> Tuple[list, Point]:
        """One GWC19 point set: the polynomials p_j ((n_j, 4) int64 torch tensors in `form`, in HBM on
        the set's device) opened at z under the challenge v -> ([p_j(z)], witness), canonical, with
        witness = sum_k q_k set[offset + k] for q = (c - c(z)) / (X - z), c = sum_j v^j p_j: one pass
        over the polynomials, one division and ONE MSM, whatever m is."""
        if self.handle is None:
            raise _lib.ArgumentError("base set is closed")
        from . import device as dv
        keep, ptrs, lens = dv.batch_tables(polys)
        stream = dv._stream_handle(keep[0].device) if keep else None
        return self.open_batch_pointers(ptrs, lens, len(keep), z, v, offset, form, stream)

    def open_batch_arrays(self, polys, z: int, v: int, offset: int = 0,
                          form: int = _lib.SV_CANONICAL) -> Tuple[list, Point]:
        """The same for host coefficients ((n_j, 4) u64 numpy arrays in `form`): uploaded with torch to
        the set's device, then the device path (the library has no host-fed batch)."""
        if self.handle is None:
            raise _lib.ArgumentError("base set is closed")
        import torch
        up = [torch.from_numpy(np.ascontiguousarray(p, dtype=np.uint64).view(np.int64)).to(f"cuda:{self.device}")
              for p in polys]
        return self.open_batch_device(up, z, v, offset=offset, form=form)


def batch_multi_scalar_multiplication(msms: Sequence[Sequence[Tuple[int, Point]]]) -> list:
    """[NativeLoader.multi_scalar_multiplication(pairs) for pairs in msms], one GPU launch."""
    offsets = [0]
    scalars, bases = [], []
    for pairs in msms:
        if len(pairs) == 0:
            raise ReferencePanic("pairs should not be empty")
        scalars += [s for s, _ in pairs]
        bases += [b for _, b in pairs]
        offsets.append(len(scalars))
    if not msms:
        return []
    return msm_batch_arrays(enc.bases_array(bases), enc.scalars_array(scalars), offsets)


class NativeLoader:
    """Mirror of snark_verifier::loader::native::NativeLoader (stateless, like the reference's
    ``lazy_static`` LOADER, native.rs:11-19)."""

    @staticmethod
    def multi_scalar_multiplication(pairs: Sequence[Tuple[int, Point]], num_gpus: int = 0) -> Point:
        if len(pairs) == 0:
            raise ReferencePanic("pairs should not be empty")
        scalars = [s for s, _ in pairs]
        bases = [b for _, b in pairs]
        return multi_scalar_multiplication(scalars, bases, num_gpus)

    @staticmethod
    def multi_scalar_multiplication_batch(msms: Sequence[Sequence[Tuple[int, Point]]]) -> list:
        return batch_multi_scalar_multiplication(msms)


def fold_partials(partials: Sequence[Tuple[int, int, int]], out_form: int = _lib.SV_CANONICAL) -> Point:
    """Fold canonical Jacobian partials (X, Y, Z) in order -> affine (host-only, no GPU)."""
    arr = (_lib.sv_g1_jacobian * len(partials))(*[enc.jacobian_struct(*p) for p in partials])
    out = _lib.sv_g1_affine()
    _lib.check(_lib.lib.sv_bn254_g1_fold(ctypes.cast(arr, ctypes.c_void_p), len(partials), ctypes.byref(out),
                                         out_form), "sv_bn254_g1_fold")
    return enc.g1_from_struct(out, out_form)
