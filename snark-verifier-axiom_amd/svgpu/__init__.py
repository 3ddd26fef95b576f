"""svgpu -- MI355X-native BN254 MSM + KZG decider behind snark-verifier's native hot-path API.

Mirrors (reference = yuliakot/snark-verifier-axiom):
  NativeLoader.multi_scalar_multiplication   snark-verifier/src/loader/native.rs:61-71
  multi_scalar_multiplication                snark-verifier/src/util/msm.rs:287-316
  KzgAs.decide / decide_all                  snark-verifier/src/pcs/kzg/decider.rs:60-80
  KzgAs.create_proof / verify (no blind)     snark-verifier/src/pcs/kzg/accumulation.rs:146-195
  Poseidon / PoseidonTranscript              snark-verifier/src/util/hash/poseidon.rs:412-467,
                                             system/halo2/transcript/halo2.rs:198-227
All compute runs in libsvgpu.so (HIP, gfx950); there is no CPU fallback.
"""
from ._lib import (SV_CANONICAL, SV_MONTGOMERY, ArgumentError, DeviceError, EmptyError, LengthError,
                   OutOfMemoryError, SvError, lib)
from .kzg import (AssertionFailure, Bdfg21Opening, KzgAccumulator, KzgAs, KzgDecidingKey, bdfg21_open,
                  bdfg21_query_sets, gwc19_open, gwc19_query_sets)
from .loader import (BaseTable, NativeLoader, ReferencePanic, ResidentBases, batch_multi_scalar_multiplication,
                     fold_partials, msm_arrays, make_refs, msm_batch_arrays, msm_refs, multi_scalar_multiplication)
from .poseidon import Poseidon, PoseidonTranscript


def init(num_devices: int = 0) -> int:
    from ._lib import check
    check(lib.sv_init(num_devices), "sv_init")
    return lib.sv_device_count()


def poly_div_linear_device(coeffs, z, **kwargs):
    """svgpu.device.poly_div_linear_device (imported on first use: that module needs torch)."""
    from .device import poly_div_linear_device as run
    return run(coeffs, z, **kwargs)


def poly_combine_eval_device(polys, z, v, **kwargs):
    """svgpu.device.poly_combine_eval_device (imported on first use: that module needs torch)."""
    from .device import poly_combine_eval_device as run
    return run(polys, z, v, **kwargs)


def poly_eval_points_device(polys, points, **kwargs):
    """svgpu.device.poly_eval_points_device (imported on first use: that module needs torch)."""
    from .device import poly_eval_points_device as run
    return run(polys, points, **kwargs)


def poly_div_roots_device(coeffs, roots, **kwargs):
    """svgpu.device.poly_div_roots_device (imported on first use: that module needs torch)."""
    from .device import poly_div_roots_device as run
    return run(coeffs, roots, **kwargs)


def root_of_unity(k: int, form: int = SV_CANONICAL) -> int:
    """omega_k, the reference's root_of_unity(k) (util/arithmetic.rs:89-96; k <= 28), as a canonical
    int.  `form` is the form the library is asked for: the value returned is the same."""
    import ctypes

    from . import encoding as enc
    from ._lib import check, sv_fe
    out = sv_fe()
    check(lib.sv_bn254_fr_root_of_unity(k, form, ctypes.byref(out)), "sv_bn254_fr_root_of_unity")
    return enc.fr_from_struct(out, form)


def ntt_device(data, **kwargs):
    """svgpu.device.ntt_device (imported on first use: that module needs torch)."""
    from .device import ntt_device as run
    return run(data, **kwargs)


def coset_lde_device(coeffs, log_ext, **kwargs):
    """svgpu.device.coset_lde_device (imported on first use: that module needs torch)."""
    from .device import coset_lde_device as run
    return run(coeffs, log_ext, **kwargs)


def quotient_coeffs_device(numer, log_n, pieces, shift, **kwargs):
    """svgpu.device.quotient_coeffs_device (imported on first use: that module needs torch)."""
    from .device import quotient_coeffs_device as run
    return run(numer, log_n, pieces, shift, **kwargs)


def extended_k(k: int, degree: int) -> int:
    """halo2's EvaluationDomain rule for the extended domain of a circuit of 2^k rows whose
    constraints have degree `degree`: the smallest K >= k with 2^K >= 2^k (degree - 1).  The quotient
    then has degree - 1 pieces of 2^k coefficients."""
    if k < 0 or degree < 2:
        raise LengthError(f"extended_k: k = {k}, degree = {degree}: a circuit has k >= 0 and degree >= 2")
    K = k
    while (1 << K) < (1 << k) * (degree - 1):
        K += 1
    return K


def commit_pieces(bases: ResidentBases, h, n: int, form: int = SV_MONTGOMERY):
    """The commitments of the quotient's pieces: h is the (pieces n, 4) tensor quotient_coeffs_device
    returns (limbs in `form`, on the set's device), piece i its rows [i n, (i + 1) n); one
    msm_bases_device per piece over set[0:n] -> a list of affine points (None = identity)."""
    rows = h.shape[0]
    if n <= 0 or rows == 0 or rows % n:
        raise LengthError(f"commit_pieces: {rows} rows are not a positive number of pieces of {n}")
    return [bases.msm_device(h[i * n:(i + 1) * n], offset=0, form=form) for i in range(rows // n)]


def grand_product_device(num, den, **kwargs):
    """svgpu.device.grand_product_device (imported on first use: that module needs torch)."""
    from .device import grand_product_device as run
    return run(num, den, **kwargs)


def batch_invert_device(data, **kwargs):
    """svgpu.device.batch_invert_device (imported on first use: that module needs torch)."""
    from .device import batch_invert_device as run
    return run(data, **kwargs)


def permutation_factors(values, sigmas, beta, gamma, delta_powers):
    """The factor lists (num, den) of one chunk of the permutation argument (system/halo2.rs:501-591):
    z(wX) prod_j (v_j + beta sigma_j + gamma) = z(X) prod_j (v_j + beta delta^j X + gamma), so row i
    multiplies z by prod_j (v_j + beta delta^j omega^i + gamma) / prod_j (v_j + beta sigma_j + gamma).
    delta_powers[j] is the delta^j of the chunk's j-th column; scalars are canonical ints."""
    from ._lib import SV_FACTOR_COLUMN, SV_FACTOR_IDENTITY
    from .encoding import R
    if not len(values) == len(sigmas) == len(delta_powers):
        raise LengthError("permutation_product: values, sigmas and delta_powers differ in length")
    num = [(SV_FACTOR_IDENTITY, v, None, beta * d % R, gamma) for v, d in zip(values, delta_powers)]
    den = [(SV_FACTOR_COLUMN, v, s, beta % R, gamma) for v, s in zip(values, sigmas)]
    return num, den


def lookup_factors(inputs, tables, permuted_input, permuted_table, beta, gamma):
    """The factor lists (num, den) of one lookup argument (system/halo2.rs:593-660):
    z(wX) (a' + beta)(s' + gamma) = z(X) (a + beta)(s + gamma) with a = inputs, s = tables (the
    compressed expressions) and a', s' their permuted columns."""
    from ._lib import SV_FACTOR_PLAIN
    num = [(SV_FACTOR_PLAIN, inputs, None, 0, beta), (SV_FACTOR_PLAIN, tables, None, 0, gamma)]
    den = [(SV_FACTOR_PLAIN, permuted_input, None, 0, beta), (SV_FACTOR_PLAIN, permuted_table, None, 0, gamma)]
    return num, den


def permutation_product(values, sigmas, beta, gamma, delta_powers, omega, z0=1, **kwargs):
    """grand_product_device over permutation_factors(...): (z, total) of one chunk; the next chunk
    takes this total as its z0."""
    num, den = permutation_factors(values, sigmas, beta, gamma, delta_powers)
    return grand_product_device(num, den, z0=z0, omega=omega, **kwargs)


def lookup_product(inputs, tables, permuted_input, permuted_table, beta, gamma, z0=1, **kwargs):
    """grand_product_device over lookup_factors(...): (z, total) of one lookup."""
    num, den = lookup_factors(inputs, tables, permuted_input, permuted_table, beta, gamma)
    return grand_product_device(num, den, z0=z0, **kwargs)


def permutation_terms_device(cols, sigmas, s, chunk, z, l0, l_last, l_active, beta, gamma, y, log_n,
                             last_rotation, **kwargs):
    """svgpu.device.permutation_terms_device (imported on first use: that module needs torch)."""
    from .device import permutation_terms_device as run
    return run(cols, sigmas, s, chunk, z, l0, l_last, l_active, beta, gamma, y, log_n, last_rotation, **kwargs)


def lookup_terms_device(lookups, l0, l_last, l_active, beta, gamma, y, log_n, **kwargs):
    """svgpu.device.lookup_terms_device (imported on first use: that module needs torch)."""
    from .device import lookup_terms_device as run
    return run(lookups, l0, l_last, l_active, beta, gamma, y, log_n, **kwargs)


def expressions_device(program, cols, consts, stores=(), **kwargs):
    """svgpu.device.expressions_device (imported on first use: that module needs torch)."""
    from .device import expressions_device as run
    return run(program, cols, consts, stores, **kwargs)


def compile_expressions(sinks):
    """svgpu.expr.compile_expressions: expression trees -> (ops, consts, depth) for expressions_device."""
    from .expr import compile_expressions as run
    return run(sinks)


def compress_expressions(exprs, theta):
    """svgpu.expr.compress_expressions: the theta-compression of a lookup's expressions as one tree."""
    from .expr import compress_expressions as run
    return run(exprs, theta)


def lagrange_selectors_device(k, log_ext, blinding, **kwargs):
    """svgpu.device.lagrange_selectors_device (imported on first use: that module needs torch)."""
    from .device import lagrange_selectors_device as run
    return run(k, log_ext, blinding, **kwargs)


def permutation_terms(values, sigmas, z, chunk, l0, l_last, l_active, beta, gamma, y, delta, log_n,
                      last_rotation, **kwargs):
    """permutation_terms_device with s_j = beta delta^j built here, as permutation_factors builds it
    for the grand product: values and sigmas are all m permutation columns on the extended domain,
    z the ceil(m / chunk) running products, delta the domain's coset generator (a canonical int)."""
    from .encoding import R
    s, d = [], 1
    for _ in values:
        s.append(beta * d % R)
        d = d * delta % R
    return permutation_terms_device(values, sigmas, s, chunk, z, l0, l_last, l_active, beta, gamma, y, log_n,
                                    last_rotation, **kwargs)


def sort_device(data, **kwargs):
    """svgpu.device.sort_device (imported on first use: that module needs torch)."""
    from .device import sort_device as run
    return run(data, **kwargs)


def lookup_permute_device(inputs, tables, **kwargs):
    """svgpu.device.lookup_permute_device (imported on first use: that module needs torch)."""
    from .device import lookup_permute_device as run
    return run(inputs, tables, **kwargs)


def lookup_argument(inputs, tables, beta, gamma, z0=1, **kwargs):
    """One lookup argument on columns in HBM: lookup_permute_device, then lookup_product over its
    output -> (permuted_input, permuted_table, z, total).  For a lookup that holds, total == z0.
    form= goes to both calls, out= (two tensors) to the permutation."""
    out = kwargs.pop("out", None)
    permuted_input, permuted_table = lookup_permute_device(inputs, tables, out=out, **kwargs)
    z, total = lookup_product(inputs, tables, permuted_input, permuted_table, beta, gamma, z0=z0, **kwargs)
    return permuted_input, permuted_table, z, total


def lookup_permute_batch_device(inputs, tables, **kwargs):
    """svgpu.device.lookup_permute_batch_device (imported on first use: that module needs torch)."""
    from .device import lookup_permute_batch_device as run
    return run(inputs, tables, **kwargs)


def lookup_arguments(inputs, tables, beta, gamma, z0=1, **kwargs):
    """The lookup arguments of a circuit on columns in HBM: one lookup_permute_batch_device over all
    of them (`tables` a list, or one tensor that every lookup shares), then lookup_product per lookup
    -> [(permuted_input, permuted_table, z, total), ..], per lookup what lookup_argument returns.
    form= goes to every call, out= (pairs of tensors) and tables_sorted= to the permutation."""
    out, tables_sorted = kwargs.pop("out", None), kwargs.pop("tables_sorted", False)
    pairs = lookup_permute_batch_device(inputs, tables, out=out, tables_sorted=tables_sorted, **kwargs)
    if not isinstance(tables, (list, tuple)):
        tables = [tables] * len(pairs)
    result = []
    for a, s, (permuted_input, permuted_table) in zip(inputs, tables, pairs):
        z, total = lookup_product(a, s, permuted_input, permuted_table, beta, gamma, z0=z0, **kwargs)
        result.append((permuted_input, permuted_table, z, total))
    return result


def version() -> str:
    return lib.sv_version().decode()
