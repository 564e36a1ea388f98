"""ctypes binding of libphyhip.so (the C ABI in include/phyhip.h).

Python is only the test / benchmark harness here; the product is the shared library.  Loading fails
loudly when the library has not been built (`python -c 'import __graft_entry__ as g; g.build()'`);
there is no fallback implementation.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PHYHIP_LIBDIR: another build of the same libraries (tools/build_diag.sh puts the -DPHYHIP_DIAG build in phyml_amd/lib_diag)
LIB_DIR = os.environ.get("PHYHIP_LIBDIR") or os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libphyhip.so")


class PhyhipError(RuntimeError):
    code = None  # the PHYHIP_ERROR_* value, where a C entry point returned one


class Operation(C.Structure):
    _fields_ = [("destinationPartials", C.c_int), ("destinationScaleWrite", C.c_int), ("destinationScaleRead", C.c_int),
                ("child1Partials", C.c_int), ("child1TransitionMatrix", C.c_int),
                ("child2Partials", C.c_int), ("child2TransitionMatrix", C.c_int)]


class RegraftCandidate(C.Structure):
    """phyhip_regraft_candidate"""
    _fields_ = [("child1Partials", C.c_int), ("child2Partials", C.c_int), ("subtreePartials", C.c_int), ("flags", C.c_int),
                ("child1Length", C.c_double), ("child2Length", C.c_double), ("subtreeLength", C.c_double)]


class ParsimonyCandidate(C.Structure):
    """phyhip_parsimony_candidate"""
    _fields_ = [("child1", C.c_int), ("child2", C.c_int), ("subtree", C.c_int)]


class TripleCandidate(C.Structure):
    """phyhip_triple_candidate"""
    _fields_ = [("partials", C.c_int * 3), ("flags", C.c_int), ("length", C.c_double * 3)]


class TripleResult(C.Structure):
    """phyhip_triple_result"""
    _fields_ = [("length", C.c_double * 3), ("lnL", C.c_double), ("dLnL", C.c_double), ("lkBegin", C.c_double * 3),
                ("evaluations", C.c_int * 3), ("status", C.c_int * 3), ("warning", C.c_int), ("reserved", C.c_int)]

    def as_tuple(self):
        """(lengths, lnL, dLnL, lkBegin, evaluations, statuses, warning): compares with == bit for bit (no NaN in a finished record)"""
        return (tuple(self.length), self.lnL, self.dLnL, tuple(self.lkBegin), tuple(self.evaluations), tuple(self.status), self.warning)


class InstanceDetails(C.Structure):
    _fields_ = [("resourceNumber", C.c_int), ("resourceName", C.c_char * 64), ("implName", C.c_char * 64),
                ("flags", C.c_long), ("computeUnits", C.c_int), ("globalMemBytes", C.c_longlong)]


# every symbol include/phyhip.h declares (tests check the library exports them all)
SYMBOLS = [
    "phyhip_create_instance", "phyhip_finalize_instance", "phyhip_get_last_error", "phyhip_set_tip_partials",
    "phyhip_set_tip_states", "phyhip_set_tip_partials_at_pattern", "phyhip_set_partials", "phyhip_set_pattern_weights", "phyhip_set_category_rates",
    "phyhip_set_category_weights", "phyhip_set_state_frequencies", "phyhip_set_eigen_decomposition",
    "phyhip_set_phyml_options", "phyhip_set_invariant_sites", "phyhip_update_transition_matrices",
    "phyhip_set_transition_matrix", "phyhip_get_transition_matrix", "phyhip_update_partials",
    "phyhip_calculate_edge_log_likelihoods", "phyhip_calculate_edge_log_likelihoods_device",
    "phyhip_get_site_log_likelihoods", "phyhip_get_site_outputs", "phyhip_get_partials", "phyhip_get_scale_factors",
    "phyhip_set_scale_factors", "phyhip_get_numerical_warning", "phyhip_update_eigen_lr",
    "phyhip_calculate_eigen_lnl_dlnl", "phyhip_calculate_eigen_lnl", "phyhip_get_dot_prod", "phyhip_set_stream",
    "phyhip_synchronize", "phyhip_profile", "phyhip_profile_read", "phyhip_calculate_mixture_log_likelihood",
    "phyhip_calculate_mixture_eigen_lnl_dlnl", "phyhip_comm_get_unique_id", "phyhip_comm_init_rank", "phyhip_comm_size",
    "phyhip_get_shard_range", "phyhip_profile_read_kernel", "phyhip_profile_read_collective", "phyhip_profile_read_traffic", "phyhip_profile_read_eigen", "phyhip_get_resident_stats", "phyhip_get_big_resident_stats", "phyhip_set_virtual_buffers", "phyhip_get_virtual_stats", "phyhip_get_deferred_stats", "phyhip_set_chained_buffers", "phyhip_get_chained_stats", "phyhip_get_record_stats", "phyhip_get_step_kind_stats", "phyhip_tip_row_bits", "phyhip_calculate_class_mixture_log_likelihood",
    "phyhip_calculate_class_mixture_eigen_lnl_dlnl", "phyhip_get_class_scale_factors", "phyhip_set_mixture_invariant_sites",
    "phyhip_calculate_edge_site_outputs_exact", "phyhip_calculate_node_state_posteriors", "phyhip_profile_read_node_posteriors",
    "phyhip_calculate_pairwise_ml_distances", "phyhip_set_pairwise_work_space", "phyhip_profile_read_pairwise",
    "phyhip_set_support_site_log_likelihoods", "phyhip_calculate_sh_support", "phyhip_get_support_alias_table", "phyhip_profile_read_support",
    "phyhip_set_parsimony", "phyhip_update_partial_parsimony", "phyhip_calculate_edge_parsimony", "phyhip_get_site_parsimony",
    "phyhip_get_partial_parsimony", "phyhip_profile_read_parsimony",
    "phyhip_calculate_regraft_parsimony", "phyhip_get_regraft_site_parsimony", "phyhip_get_regraft_partial_parsimony",
    "phyhip_profile_read_regraft_parsimony",
    "phyhip_optimise_edge_length", "phyhip_profile_read_edge_length",
    "phyhip_calculate_regraft_log_likelihoods", "phyhip_get_regraft_partials", "phyhip_get_regraft_transition_matrix",
    "phyhip_set_regraft_work_space", "phyhip_profile_read_regraft",
    "phyhip_calculate_mixture_regraft_log_likelihoods", "phyhip_get_mixture_regraft_partials",
    "phyhip_get_mixture_regraft_transition_matrix", "phyhip_set_mixture_regraft_work_space", "phyhip_profile_read_mixture_regraft",
    "phyhip_optimise_triples", "phyhip_get_triple_partials", "phyhip_set_triple_work_space", "phyhip_profile_read_triples",
]

FLAG_SHARDED = 1 << 40  # PHYHIP_FLAG_SHARDED
FLAG_CLASS_AXIS = 1 << 41  # PHYHIP_FLAG_CLASS_AXIS
UNIQUE_ID_BYTES = 128
PARS_TILE = 256  # kParsTile of phyml_amd/csrc/phyhip_pars.hip: patterns per workgroup of the parsimony kernels
PARS_STAGING = 4096  # kParsStaging: operations one parsimony launch takes (a longer queue is launched as it fills)
MAX_PARS = 1000000000  # src/utilities.h
PARS_REGRAFT_SLAB_FACTOR = 8  # kParsScanSlabFactor of phyml_amd/csrc/phyhip_scan_plan.hpp
PARS_REGRAFT_CHUNK = 65535  # kScanGridCap: candidates of one launch of regraft_parsimony
PARS_REGRAFT_LDS = {"fitch": 32, "general": 64}  # kParsScanFitchLds, kParsScanGeneralLds (the step-matrix kernel: plus S * S ints)


def pars_regraft_slabs(count, P, compute_units, factor=PARS_REGRAFT_SLAB_FACTOR):
    """(slabs, records per slab) of one launch of regraft_parsimony over `count` <= PARS_REGRAFT_CHUNK candidates, as ParsScanSlabs
    (phyml_amd/csrc/phyhip_scan_plan.hpp) cuts it: enough slabs to give every compute unit `factor` workgroups, no more than
    candidates; every slab but the last holds that many records.  compute_units: Instance.details.computeUnits."""
    if count == 0:
        return 0, 0
    tiles = max(1, (P + PARS_TILE - 1) // PARS_TILE)
    want = min(count, max(1, (factor * compute_units + tiles - 1) // tiles))
    size = (count + want - 1) // want
    return (count + size - 1) // size, size
ERROR_UNINITIALIZED_INSTANCE, ERROR_OUT_OF_RANGE, ERROR_NO_IMPLEMENTATION = -4, -5, -7
ERROR_FLOATING_POINT = -8
REGRAFT_SUBTREE_IS_LEFT = 1  # PHYHIP_REGRAFT_SUBTREE_IS_LEFT
REGRAFT_TILE = 256  # kRegraftTile of phyml_amd/csrc/phyhip_regraft.hip: patterns per workgroup of the scan kernel
REGRAFT_WORK_BYTES = 128 << 20  # kRegraftWorkBytes: the default bound on the scan's work space
REGRAFT_MAX_CATEGORIES = 8  # kRegraftMaxCategories: instances of more categories are refused


def regraft_chunk_candidates(P, C, S, max_bytes=REGRAFT_WORK_BYTES):
    """candidates per chunk of regraft_log_likelihoods under a work-space bound, as include/phyhip.h states the layout: the kept
    vector (P C S doubles, P ints rounded up to a multiple of 8 bytes), then per candidate 3 C S S doubles, a double per tile of
    256 patterns and 72 bytes; at least one, at most 65535 (a grid's second dimension)"""
    fixed = P * C * S * 8 + ((P + 1) // 2 * 2) * 4
    per = 3 * C * S * S * 8 + (P + REGRAFT_TILE - 1) // REGRAFT_TILE * 8 + 72
    return max(1, min(65535, (max_bytes - fixed) // per if max_bytes > fixed + per else 1))


MIXTURE_REGRAFT_CLASS_BYTES = 128  # sizeof(MixRegraftClass): an entry of the mixture scan's per-class table
MIXTURE_REGRAFT_HEAD_BYTES = 200  # sizeof(MixRegraftHead): the combination's sums and the +I share, in front of that table


def mixture_regraft_chunk_candidates(P, classes, S, max_bytes=REGRAFT_WORK_BYTES):
    """candidates per chunk of mixture_regraft_log_likelihoods under a work-space bound, as include/phyhip.h states the layout: per
    class the kept vector (P S doubles, P ints rounded up to a multiple of 8 bytes) and 128 bytes of the per-class table, the 200
    bytes in front of that table, then per candidate 3 S S doubles a class, a double per tile of 256 patterns and 72 bytes; at
    least one, at most 65535"""
    fixed = classes * (P * S * 8 + ((P + 1) // 2 * 2) * 4 + MIXTURE_REGRAFT_CLASS_BYTES) + MIXTURE_REGRAFT_HEAD_BYTES
    per = 3 * classes * S * S * 8 + (P + REGRAFT_TILE - 1) // REGRAFT_TILE * 8 + 72
    return max(1, min(65535, (max_bytes - fixed) // per if max_bytes > fixed + per else 1))


BRENT_IT_MAX = 1000  # kBrentItMax of phyml_amd/csrc/phyhip_brlen.hip (src/utilities.h:337)
BRLEN_MAX_PATTERNS = 16384  # kBrlenMaxPatterns: phyhip_optimise_edge_length refuses instances of more patterns (built and tested up to here; not where it is faster)
BRLEN_THREADS = {4: 1024, 20: 512}  # kBrlenThreads<S>: the one workgroup of the search kernel
BRLEN_KEEP = {4: 3, 20: 1}  # kBrlenKeep<S>: rounds of a lane whose inputs stay in registers across the probes

TRIPLE_MAX_PATTERNS = 16384  # kTripleMaxPatterns: phyhip_optimise_triples refuses instances of more patterns
TRIPLE_THREADS = {4: 512, 20: 256}  # kTripleThreads<S>: the workgroup of a candidate
TRIPLE_KEEP = {4: 5, 20: 2}  # kTripleKeep<S>: rounds of a search lane whose inputs stay in registers across the probes
TRIPLE_LK_END = 8  # the status of a search whose lk_end fell below lk_begin - tol (src/optimiz.c:656)


def triple_node_is_left(i):
    """PHYHIP_TRIPLE_NODE_IS_LEFT(i)"""
    return 1 << i


def triple_chunk_candidates(P, C, S, max_bytes=REGRAFT_WORK_BYTES):
    """candidates per chunk of optimise_triples under a work-space bound, as include/phyhip.h states the layout: the three kept
    vectors (P C S doubles and P ints rounded up to even each, the whole rounded up to 256 bytes), then per candidate 3 C S S + P C S
    doubles, P ints rounded up to even and 136 bytes; at least one"""
    pe = (P + 1) // 2 * 2
    fixed = (3 * (P * C * S * 8 + pe * 4) + 255) // 256 * 256
    per = (3 * C * S * S + P * C * S) * 8 + pe * 4 + 136
    return max(1, (max_bytes - fixed) // per if max_bytes > fixed + per else 1)


_lib = None


def comm_get_unique_id() -> bytes:
    """phyhip_comm_get_unique_id (rank 0; broadcast the bytes to the other ranks)."""
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    _chk(load().phyhip_comm_get_unique_id(buf))
    return buf.raw


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PhyhipError(f"{LIB_PATH} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        L = C.CDLL(LIB_PATH)
        L.phyhip_get_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def tip_row_bits(codes):
    """phyhip_tip_row_bits of a nucleotide tip row given as state-set bytes: bit 0 every code is one-hot, bit 1 some code is 15
    (host arithmetic: needs no device)"""
    a = np.ascontiguousarray(codes, dtype=np.uint8)
    return int(load().phyhip_tip_row_bits(a.ctypes.data_as(C.c_void_p), C.c_longlong(a.size)))


def _chk(rc):
    if rc < 0:
        e = PhyhipError(f"phyhip error {rc}: {load().phyhip_get_last_error().decode()}")
        e.code = rc
        raise e
    return rc


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Instance:
    """Thin object wrapper: one method per C entry point, numpy in / numpy out."""

    def __init__(self, tip_count, partials_buffer_count, state_count, pattern_count, matrix_buffer_count,
                 category_count, device=None, devices=None, force_sharded=False, class_axis=False):
        L = load()
        self.L = L
        self.tips, self.nbuf, self.S, self.P, self.nmat, self.C = (tip_count, partials_buffer_count, state_count,
                                                                  pattern_count, matrix_buffer_count, category_count)
        self.details = InstanceDetails()
        if devices is not None:  # sharded instance: one pattern range per listed device, RCCL all-reduce inside the library
            res, nres = (C.c_int * len(devices))(*[int(d) for d in devices]), len(devices)
        else:
            res, nres = ((C.c_int * 1)(device), 1) if device is not None else (None, 0)
        self.id = _chk(L.phyhip_create_instance(tip_count, partials_buffer_count, 0, state_count, pattern_count, 1,
                                                matrix_buffer_count, category_count, 0, res, nres,
                                                C.c_long(0), C.c_long((FLAG_SHARDED if force_sharded else 0) | (FLAG_CLASS_AXIS if class_axis else 0)),
                                                C.byref(self.details)))

    def close(self):
        if self.id is not None:
            self.L.phyhip_finalize_instance(self.id)
            self.id = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs
    def set_tip_partials(self, tip, partials):
        a = _f64(partials); assert a.size == self.P * self.S
        _chk(self.L.phyhip_set_tip_partials(self.id, tip, _ptr(a)))

    def set_tip_partials_at_pattern(self, tip, pattern, partials):
        a = _f64(partials); assert a.size == self.S
        _chk(self.L.phyhip_set_tip_partials_at_pattern(self.id, int(tip), int(pattern), _ptr(a)))

    def set_tip_states(self, tip, states):
        a = np.ascontiguousarray(states, dtype=np.int32); assert a.size == self.P
        _chk(self.L.phyhip_set_tip_states(self.id, tip, _ptr(a)))

    def set_partials(self, buf, partials):
        a = _f64(partials); assert a.size == self.P * self.C * self.S
        _chk(self.L.phyhip_set_partials(self.id, buf, _ptr(a)))

    def set_pattern_weights(self, w):
        a = _f64(w); assert a.size == self.P
        _chk(self.L.phyhip_set_pattern_weights(self.id, _ptr(a)))

    def set_category_rates(self, r):
        a = _f64(r); assert a.size == self.C
        _chk(self.L.phyhip_set_category_rates(self.id, _ptr(a)))

    def set_category_weights(self, w):
        a = _f64(w); assert a.size == self.C
        _chk(self.L.phyhip_set_category_weights(self.id, 0, _ptr(a)))

    def set_state_frequencies(self, pi, index=0):
        a = _f64(pi); assert a.size == self.S
        _chk(self.L.phyhip_set_state_frequencies(self.id, int(index), _ptr(a)))

    def set_eigen_decomposition(self, evec, ivec, evals, index=0):
        a, b, c = _f64(evec), _f64(ivec), _f64(evals)
        assert a.size == self.S * self.S and b.size == self.S * self.S and c.size == self.S
        _chk(self.L.phyhip_set_eigen_decomposition(self.id, int(index), _ptr(a), _ptr(b), _ptr(c)))

    # -- mixtures on the class axis (instance created with class_axis=True)
    def class_mixture_log_likelihood(self, parent, child, pm, proba, r_w, e_w, r_sum, e_sum, sum_probas):
        n = self.C
        da = lambda v: (C.c_double * n)(*[float(x) for x in v])
        out = C.c_double(0.0)
        _chk(self.L.phyhip_calculate_class_mixture_log_likelihood(self.id, int(parent), int(child), int(pm), da(proba), da(r_w), da(e_w),
                                                                 C.c_double(r_sum), C.c_double(e_sum), C.c_double(sum_probas), C.byref(out)))
        return out.value

    def class_mixture_eigen_lnl_dlnl(self, left, right, l, proba, r_w, e_w, r_sum, e_sum, sum_probas):
        n = self.C
        da = lambda v: (C.c_double * n)(*[float(x) for x in v])
        lv, lnl, dlnl = C.c_double(l), C.c_double(0.0), C.c_double(0.0)
        _chk(self.L.phyhip_calculate_class_mixture_eigen_lnl_dlnl(self.id, int(left), int(right), C.byref(lv), da(proba), da(r_w), da(e_w),
                                                                 C.c_double(r_sum), C.c_double(e_sum), C.c_double(sum_probas),
                                                                 C.byref(lnl), C.byref(dlnl)))
        return lv.value, lnl.value, dlnl.value

    def get_class_scale_factors(self, buf, k):
        out = np.zeros(self.P, np.int32)
        _chk(self.L.phyhip_get_class_scale_factors(self.id, int(buf), int(k), _ptr(out)))
        return out

    def set_phyml_options(self, l_min=1e-8, l_max=100.0, br_len_mult=1.0, apply_lk_scaling=1):
        _chk(self.L.phyhip_set_phyml_options(self.id, C.c_double(l_min), C.c_double(l_max), C.c_double(br_len_mult),
                                             int(apply_lk_scaling)))

    def set_invariant_sites(self, invar_model, pinvar, invar):
        a = None if invar is None else np.ascontiguousarray(invar, dtype=np.int16)
        _chk(self.L.phyhip_set_invariant_sites(self.id, int(invar_model), C.c_double(pinvar), _ptr(a)))

    # -- matrices
    def update_transition_matrices(self, indices, lengths):
        i = np.ascontiguousarray(indices, dtype=np.int32); l = _f64(lengths); assert i.size == l.size
        _chk(self.L.phyhip_update_transition_matrices(self.id, 0, _ptr(i), None, None, _ptr(l), int(i.size)))

    def set_transition_matrix(self, idx, mat):
        a = _f64(mat); assert a.size == self.C * self.S * self.S
        _chk(self.L.phyhip_set_transition_matrix(self.id, int(idx), _ptr(a), C.c_double(0.0)))

    def get_transition_matrix(self, idx):
        out = np.zeros((self.C, self.S, self.S))
        _chk(self.L.phyhip_get_transition_matrix(self.id, int(idx), _ptr(out)))
        return out

    # -- hot path
    def update_partials(self, ops):
        """ops: iterable of (dest, child1, pm1, child2, pm2)."""
        ops = list(ops)
        arr = (Operation * len(ops))()
        for k, (d, c1, m1, c2, m2) in enumerate(ops):
            arr[k] = Operation(d, -1, -1, c1, m1, c2, m2)
        _chk(self.L.phyhip_update_partials(self.id, arr, len(ops), -1))

    def edge_lnl(self, parent, child, pm):
        out = C.c_double(0)
        p = (C.c_int * 1)(parent); c = (C.c_int * 1)(child); m = (C.c_int * 1)(pm); z = (C.c_int * 1)(0)
        _chk(self.L.phyhip_calculate_edge_log_likelihoods(self.id, p, c, m, None, None, z, z, None, 1, C.byref(out), None, None))
        return out.value

    def edge_lnl_device(self, parent, child, pm, device_ptr):
        _chk(self.L.phyhip_calculate_edge_log_likelihoods_device(self.id, parent, child, pm, C.c_void_p(device_ptr)))

    def site_log_likelihoods(self):
        out = np.zeros(self.P)
        _chk(self.L.phyhip_get_site_log_likelihoods(self.id, _ptr(out)))
        return out

    def site_outputs(self, n_fact=1):
        """n_fact: class-axis instances return fact_sum_scale as [class][pattern] (n_fact = class count)."""
        a = np.zeros(self.P); b = np.zeros(self.P); c = np.zeros((self.P, self.C)); f = np.zeros(self.P * n_fact, np.int32)
        _chk(self.L.phyhip_get_site_outputs(self.id, _ptr(a), _ptr(b), _ptr(c), _ptr(f)))
        return a, b, c, f

    def exact_site_outputs(self, parent, child, pmat):
        """phyhip_calculate_edge_site_outputs_exact: (c_lnL_sorted, cur_site_lk, unscaled_site_lk_cat, fact_sum_scale, ordered
        sum, numerical warning) of the edge as the reference's doubles; nothing the last evaluation left is touched."""
        a = np.zeros(self.P); b = np.zeros(self.P); c = np.zeros((self.P, self.C)); f = np.zeros(self.P, np.int32)
        s = C.c_double(0.0); w = C.c_int(0)
        _chk(self.L.phyhip_calculate_edge_site_outputs_exact(self.id, int(parent), int(child), int(pmat), _ptr(a), _ptr(b), _ptr(c),
                                                             _ptr(f), C.byref(s), C.byref(w)))
        return a, b, c, f, s.value, w.value

    def node_state_posteriors(self, sides, matrices, site_lnl=None, with_warning=False):
        """phyhip_calculate_node_state_posteriors: the marginal state posteriors [node][pattern][state] of the internal nodes whose
        three (side buffer or tip, matrix) pairs are the rows of `sides` / `matrices` ([node][3]); site_lnl: c_lnL_sorted, or None
        for what the instance's last edge evaluation left on the device.  with_warning: (posteriors, numerical warning)."""
        s = np.ascontiguousarray(sides, dtype=np.int32).reshape(-1, 3); m = np.ascontiguousarray(matrices, dtype=np.int32).reshape(-1, 3)
        assert s.shape == m.shape
        l = None if site_lnl is None else _f64(site_lnl)
        assert l is None or l.size == self.P
        out = np.zeros((s.shape[0], self.P, self.S)); w = C.c_int(0)
        _chk(self.L.phyhip_calculate_node_state_posteriors(self.id, int(s.shape[0]), _ptr(s), _ptr(m), _ptr(l), _ptr(out), C.byref(w)))
        return (out, w.value) if with_warning else out

    def profile_read_node_posteriors(self):
        """(ms, calls) of the kernel of node_state_posteriors since the previous read, while profile(1)"""
        ms = C.c_double(0); n = C.c_int(0)
        _chk(self.L.phyhip_profile_read_node_posteriors(self.id, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def pairwise_ml_distances(self, min_diff_lk=1e-3, initial=None, eigen_index=0, frequencies_index=0, want=()):
        """phyhip_calculate_pairwise_ml_distances: the [tip][tip] ML distance matrix (ML_Dist).  initial: K80_dist's / JC69_Dist's
        matrix, or None for the closed form from the device's counts.  want: any of "initial" ([tip][tip], before the 0.1 rule),
        "counts" ([pair][state][state] normalised F), "lnl" ([pair]), "iterations" ([pair]); with a non-empty `want` the result is
        (distances, {name: array})."""
        n, npair = self.tips, self.tips * (self.tips - 1) // 2
        bad = set(want) - {"initial", "counts", "lnl", "iterations"}
        assert not bad, bad
        ini = None if initial is None else _f64(initial)
        assert ini is None or ini.size == n * n
        out = np.zeros((n, n))
        extra = {}
        if "initial" in want: extra["initial"] = np.zeros((n, n))
        if "counts" in want: extra["counts"] = np.zeros((npair, self.S, self.S))
        if "lnl" in want: extra["lnl"] = np.zeros(npair)
        if "iterations" in want: extra["iterations"] = np.zeros(npair, np.int32)
        fn = self.L.phyhip_calculate_pairwise_ml_distances
        fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 6
        _chk(fn(self.id, int(eigen_index), int(frequencies_index), float(min_diff_lk), _ptr(ini), _ptr(out), _ptr(extra.get("initial")),
                _ptr(extra.get("counts")), _ptr(extra.get("lnl")), _ptr(extra.get("iterations"))))
        return (out, extra) if want else out

    def set_pairwise_work_space(self, max_bytes):
        """phyhip_set_pairwise_work_space: bytes of raw counts pairwise_ml_distances holds at a time (0: the default)"""
        _chk(self.L.phyhip_set_pairwise_work_space(self.id, C.c_longlong(int(max_bytes))))

    def profile_read_pairwise(self):
        """(count kernels ms, optimiser kernels ms, calls) of pairwise_ml_distances since the previous read, while profile(1)"""
        a = C.c_double(0); b = C.c_double(0); n = C.c_int(0)
        _chk(self.L.phyhip_profile_read_pairwise(self.id, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def set_support_site_lnl(self, slot, site_lnl=None):
        """phyhip_set_support_site_log_likelihoods: slot 0..2 of the SH-like support's three per-pattern vectors (log_lks_aLRT);
        site_lnl None: what the last edge evaluation left on the device, copied device to device."""
        a = None if site_lnl is None else _f64(site_lnl)
        assert a is None or a.size == self.P
        fn = self.L.phyhip_set_support_site_log_likelihoods
        fn.argtypes = [C.c_int, C.c_int, C.c_void_p]
        _chk(fn(self.id, int(slot), _ptr(a)))

    def sh_support(self, site_count, replicates=10000, seed=0, want=()):
        """phyhip_calculate_sh_support: (SH-like support, RELL support, totals c_0..c_2) of the three slots under the instance's
        pattern weights (Statistics_To_SH / Statistics_to_RELL).  want: any of "sums" ([replicate][3], uncentred), "accepted"
        ([replicate] 0 / 1); with a non-empty `want` the result is (sh, rell, totals, {name: array})."""
        bad = set(want) - {"sums", "accepted"}
        assert not bad, bad
        sh = C.c_double(0); rell = C.c_double(0); tot = np.zeros(3)
        extra = {}
        if "sums" in want: extra["sums"] = np.zeros((int(replicates), 3))
        if "accepted" in want: extra["accepted"] = np.zeros(int(replicates), np.int32)
        fn = self.L.phyhip_calculate_sh_support
        fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong] + [C.c_void_p] * 5
        _chk(fn(self.id, int(site_count), int(replicates), int(seed) & 0xFFFFFFFFFFFFFFFF, C.cast(C.byref(sh), C.c_void_p),
                C.cast(C.byref(rell), C.c_void_p), _ptr(tot), _ptr(extra.get("sums")), _ptr(extra.get("accepted"))))
        return (sh.value, rell.value, tot, extra) if want else (sh.value, rell.value, tot)

    def support_alias_table(self, site_count):
        """phyhip_get_support_alias_table: (prob, alias) of Sample_n_i_With_Proba_pi for the instance's weights and site_count"""
        prob = np.zeros(self.P); alias = np.zeros(self.P, np.int32)
        fn = self.L.phyhip_get_support_alias_table
        fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _chk(fn(self.id, int(site_count), _ptr(prob), _ptr(alias)))
        return prob, alias

    def profile_read_support(self):
        """(kernel ms, calls) of sh_support since the previous read, while profile(1)"""
        ms = C.c_double(0); n = C.c_int(0)
        _chk(self.L.phyhip_profile_read_support(self.id, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- parsimony (src/pars.c)
    def set_parsimony(self, general=False, step_matrix=None):
        """phyhip_set_parsimony: Fitch mode, or -- general -- the step-matrix mode with step_matrix [S][S] (row = parent state)"""
        m = None if step_matrix is None else np.ascontiguousarray(step_matrix, dtype=np.int32)
        assert m is None or m.size == self.S * self.S
        _chk(self.L.phyhip_set_parsimony(self.id, 1 if general else 0, _ptr(m)))

    def update_partial_parsimony(self, ops):
        """phyhip_update_partial_parsimony: ops = iterable of (dest, child1, child2), queued"""
        a = np.ascontiguousarray(np.array(list(ops), dtype=np.int32).reshape(-1, 3))
        _chk(self.L.phyhip_update_partial_parsimony(self.id, _ptr(a), int(a.shape[0])))

    def edge_parsimony(self, buffer1, buffer2, with_sum=True):
        """phyhip_calculate_edge_parsimony: the queue, then the score of the edge (buffer1, buffer2): the 64-bit weighted sum, or
        None with with_sum=False (per-pattern scores only)"""
        out = C.c_longlong(0)
        _chk(self.L.phyhip_calculate_edge_parsimony(self.id, int(buffer1), int(buffer2), C.byref(out) if with_sum else None))
        return out.value if with_sum else None

    def site_parsimony(self):
        out = np.zeros(self.P, np.int32)
        _chk(self.L.phyhip_get_site_parsimony(self.id, _ptr(out)))
        return out

    def partial_parsimony(self, buf, general=False):
        """phyhip_get_partial_parsimony: (ui, pars) of the buffer, or -- general -- p_pars [pattern][state]"""
        if general:
            pp = np.zeros((self.P, self.S), np.int32)
            _chk(self.L.phyhip_get_partial_parsimony(self.id, int(buf), None, None, _ptr(pp)))
            return pp
        ui = np.zeros(self.P, np.int32); pars = np.zeros(self.P, np.int32)
        _chk(self.L.phyhip_get_partial_parsimony(self.id, int(buf), _ptr(ui), _ptr(pars), None))
        return ui, pars

    def profile_read_parsimony(self):
        """(kernel ms, launches, pattern updates) of the parsimony kernels since the previous read, while profile(1)"""
        ms = C.c_double(0); n = C.c_int(0); u = C.c_double(0)
        _chk(self.L.phyhip_profile_read_parsimony(self.id, C.byref(ms), C.byref(n), C.byref(u)))
        return ms.value, n.value, u.value

    # -- parsimony regraft scan (src/spr.c: Test_One_Spr_Target under spr_pars)
    def regraft_parsimony(self, candidates, keep=-1):
        """phyhip_calculate_regraft_parsimony: candidates = iterable of (child1, child2, subtree), or a prebuilt ParsimonyCandidate
        array; keep: the candidate whose joined vector and site scores stay for the two getters.  Returns the sums [K] (int64)."""
        if isinstance(candidates, C.Array):
            arr, n = candidates, len(candidates)
        else:
            a = np.ascontiguousarray(np.array(list(candidates), dtype=np.int32).reshape(-1, 3))
            n = int(a.shape[0])
            arr = (ParsimonyCandidate * max(1, n)).from_buffer_copy(a.tobytes() if n else bytes(12))
        out = np.zeros(n, np.int64)
        _chk(self.L.phyhip_calculate_regraft_parsimony(self.id, arr, n, int(keep), _ptr(out)))
        return out

    def regraft_site_parsimony(self):
        """phyhip_get_regraft_site_parsimony: the kept candidate's per-pattern scores"""
        out = np.zeros(self.P, np.int32)
        _chk(self.L.phyhip_get_regraft_site_parsimony(self.id, _ptr(out)))
        return out

    def regraft_partial_parsimony(self, general=False):
        """phyhip_get_regraft_partial_parsimony: (ui, pars) of the kept candidate's joined vector, or -- general -- p_pars [pattern][state]"""
        if general:
            pp = np.zeros((self.P, self.S), np.int32)
            _chk(self.L.phyhip_get_regraft_partial_parsimony(self.id, None, None, _ptr(pp)))
            return pp
        ui = np.zeros(self.P, np.int32); pars = np.zeros(self.P, np.int32)
        _chk(self.L.phyhip_get_regraft_partial_parsimony(self.id, _ptr(ui), _ptr(pars), None))
        return ui, pars

    def profile_read_regraft_parsimony(self):
        """(kernel ms, calls, candidates) of the parsimony regraft scans since the previous read, while profile(1)"""
        ms = C.c_double(0); n = C.c_int(0); nc = C.c_longlong(0)
        _chk(self.L.phyhip_profile_read_regraft_parsimony(self.id, C.byref(ms), C.byref(n), C.byref(nc)))
        return ms.value, n.value, nc.value

    def get_partials(self, buf):
        out = np.zeros((self.P, self.C * self.S))
        _chk(self.L.phyhip_get_partials(self.id, int(buf), -1, _ptr(out)))
        return out

    def get_scale_factors(self, buf):
        out = np.zeros(self.P, np.int32)
        _chk(self.L.phyhip_get_scale_factors(self.id, int(buf), _ptr(out)))
        return out

    def numerical_warning(self):
        w = C.c_int(0)
        _chk(self.L.phyhip_get_numerical_warning(self.id, C.byref(w)))
        return w.value

    # -- eigen basis
    def update_eigen_lr(self, left, rght):
        _chk(self.L.phyhip_update_eigen_lr(self.id, int(left), int(rght)))

    def eigen_lnl_dlnl(self, l):
        lv = C.c_double(l); a = C.c_double(0); b = C.c_double(0)
        _chk(self.L.phyhip_calculate_eigen_lnl_dlnl(self.id, C.byref(lv), C.byref(a), C.byref(b)))
        return lv.value, a.value, b.value

    def optimise_edge_length(self, l, init_lnl, iter_max=BRENT_IT_MAX, tol=1e-3):
        """phyhip_optimise_edge_length: Br_Len_Spline on the products update_eigen_lr left, one device call.
        Returns (l, lnL, dlnL, evaluations, status)."""
        lv = C.c_double(l); a = C.c_double(0); b = C.c_double(0); n = C.c_int(0); st = C.c_int(0)
        _chk(self.L.phyhip_optimise_edge_length(self.id, C.byref(lv), C.c_double(init_lnl), int(iter_max), C.c_double(tol),
                                                C.byref(a), C.byref(b), C.byref(n), C.byref(st)))
        return lv.value, a.value, b.value, n.value, st.value

    def profile_read_edge_length(self):
        """(kernel ms, calls, evaluations) of the edge-length searches since the previous read, while profile(1)"""
        ms = C.c_double(0); n = C.c_int(0); ev = C.c_longlong(0)
        _chk(self.L.phyhip_profile_read_edge_length(self.id, C.byref(ms), C.byref(n), C.byref(ev)))
        return ms.value, n.value, ev.value

    # -- regraft scan (src/spr.c: Test_One_Spr_Target)
    def regraft_log_likelihoods(self, candidates, keep=-1, eigen_index=0, with_warnings=False):
        """phyhip_calculate_regraft_log_likelihoods: candidates = iterable of (child1, child2, subtree, flags, child1 length,
        child2 length, subtree length); keep: the candidate whose computed vector stays for regraft_partials().  Returns the
        log-likelihoods [K], or (log-likelihoods, warnings [K]) with with_warnings."""
        cand = list(candidates)
        arr = (RegraftCandidate * max(1, len(cand)))()
        for k, (c1, c2, sub, flags, l1, l2, l3) in enumerate(cand):
            arr[k] = RegraftCandidate(int(c1), int(c2), int(sub), int(flags), float(l1), float(l2), float(l3))
        out = np.zeros(len(cand)); w = np.zeros(len(cand), np.int32)
        _chk(self.L.phyhip_calculate_regraft_log_likelihoods(self.id, int(eigen_index), arr, len(cand), int(keep), _ptr(out), _ptr(w)))
        return (out, w) if with_warnings else out

    def regraft_partials(self):
        """phyhip_get_regraft_partials: (vector [P][C*S], scale exponents [P]) of the kept candidate of the last scan"""
        v = np.zeros((self.P, self.C * self.S)); s = np.zeros(self.P, np.int32)
        _chk(self.L.phyhip_get_regraft_partials(self.id, _ptr(v), _ptr(s)))
        return v, s

    def regraft_transition_matrix(self, candidate, which):
        """phyhip_get_regraft_transition_matrix: matrix 0 (child 1), 1 (child 2) or 2 (subtree) of a candidate of the last scan"""
        out = np.zeros((self.C, self.S, self.S))
        _chk(self.L.phyhip_get_regraft_transition_matrix(self.id, int(candidate), int(which), _ptr(out)))
        return out

    def set_regraft_work_space(self, max_bytes):
        """phyhip_set_regraft_work_space: the bound on the scan's work space in bytes (0: the default)"""
        _chk(self.L.phyhip_set_regraft_work_space(self.id, C.c_longlong(int(max_bytes))))

    # -- three-edge length search (src/utilities.c: Triple_Dist)
    def optimise_triples(self, candidates, keep=-1, iter_max=BRENT_IT_MAX, tol=1e-3):
        """phyhip_optimise_triples: candidates = iterable of ((outer vector 0, 1, 2), flags, (length 0, 1, 2)); keep: the candidate
        whose three vectors stay for triple_partials().  Returns the list of TripleResult records."""
        cand = list(candidates)
        arr = (TripleCandidate * max(1, len(cand)))()
        for k, (x, flags, ln) in enumerate(cand):
            arr[k] = TripleCandidate((C.c_int * 3)(*[int(v) for v in x]), int(flags), (C.c_double * 3)(*[float(v) for v in ln]))
        out = (TripleResult * max(1, len(cand)))()
        _chk(self.L.phyhip_optimise_triples(self.id, arr, len(cand), int(iter_max), C.c_double(tol), int(keep), out))
        return [out[k] for k in range(len(cand))]

    def triple_partials(self, which):
        """phyhip_get_triple_partials: (vector [P][C*S], scale exponents [P]) I_which of the kept candidate of the last call"""
        v = np.zeros((self.P, self.C * self.S)); s = np.zeros(self.P, np.int32)
        _chk(self.L.phyhip_get_triple_partials(self.id, int(which), _ptr(v), _ptr(s)))
        return v, s

    def set_triple_work_space(self, max_bytes):
        """phyhip_set_triple_work_space: the bound on the call's work space in bytes (0: the default)"""
        _chk(self.L.phyhip_set_triple_work_space(self.id, C.c_longlong(int(max_bytes))))

    def profile_read_triples(self):
        """(kernel ms, calls, evaluations) of the optimise_triples calls since the previous read, while profile(1)"""
        ms = C.c_double(); n = C.c_int(); ev = C.c_longlong()
        _chk(self.L.phyhip_profile_read_triples(self.id, C.byref(ms), C.byref(n), C.byref(ev)))
        return ms.value, n.value, ev.value

    # -- regraft scan of a mixture: what the FIRST class instance keeps (mixture_regraft_log_likelihoods below)
    def mixture_regraft_partials(self, class_index):
        """phyhip_get_mixture_regraft_partials: (vector [P][S], scale exponents [P]) of class class_index of the kept candidate of the
        last mixture scan whose first instance this is"""
        v = np.zeros((self.P, self.S)); s = np.zeros(self.P, dtype=np.int32)
        _chk(self.L.phyhip_get_mixture_regraft_partials(self.id, int(class_index), _ptr(v), _ptr(s)))
        return v, s

    def mixture_regraft_transition_matrix(self, class_index, candidate, which):
        """phyhip_get_mixture_regraft_transition_matrix: matrix 0 (child 1), 1 (child 2) or 2 (subtree) of a class and a candidate of
        the last mixture scan"""
        out = np.zeros((self.S, self.S))
        _chk(self.L.phyhip_get_mixture_regraft_transition_matrix(self.id, int(class_index), int(candidate), int(which), _ptr(out)))
        return out

    def set_mixture_regraft_work_space(self, max_bytes):
        """phyhip_set_mixture_regraft_work_space: the bound on the mixture scan's work space in bytes (0: the default)"""
        _chk(self.L.phyhip_set_mixture_regraft_work_space(self.id, C.c_longlong(int(max_bytes))))

    def profile_read_mixture_regraft(self):
        """(kernel ms, calls, candidates) of the mixture regraft scans since the previous read, while profile(1)"""
        ms = C.c_double(0); n = C.c_int(0); nc = C.c_longlong(0)
        _chk(self.L.phyhip_profile_read_mixture_regraft(self.id, C.byref(ms), C.byref(n), C.byref(nc)))
        return ms.value, n.value, nc.value

    def profile_read_regraft(self):
        """(kernel ms, calls, candidates) of the regraft scans since the previous read, while profile(1)"""
        ms = C.c_double(0); n = C.c_int(0); nc = C.c_longlong(0)
        _chk(self.L.phyhip_profile_read_regraft(self.id, C.byref(ms), C.byref(n), C.byref(nc)))
        return ms.value, n.value, nc.value

    def eigen_lnl(self, l):
        a = C.c_double(0)
        _chk(self.L.phyhip_calculate_eigen_lnl(self.id, C.c_double(l), C.byref(a)))
        return a.value

    def get_dot_prod(self):
        out = np.zeros((self.P, self.C * self.S))
        _chk(self.L.phyhip_get_dot_prod(self.id, _ptr(out)))
        return out

    # -- multi-GPU
    def comm_init_rank(self, nranks, rank, unique_id: bytes):
        assert len(unique_id) == UNIQUE_ID_BYTES
        _chk(self.L.phyhip_comm_init_rank(self.id, int(nranks), int(rank), C.c_char_p(unique_id)))

    def comm_size(self):
        n = C.c_int(0)
        _chk(self.L.phyhip_comm_size(self.id, C.byref(n)))
        return n.value

    def shard_ranges(self):
        """[(device, first pattern, pattern count)] of the instance's shards."""
        out, k, n = [], 0, 1
        while k < n:
            d, lo, cnt = C.c_int(0), C.c_int(0), C.c_int(0)
            n = _chk(self.L.phyhip_get_shard_range(self.id, k, C.byref(d), C.byref(lo), C.byref(cnt)))
            out.append((d.value, lo.value, cnt.value))
            k += 1
        return out

    # -- plumbing
    def set_stream(self, stream_handle):
        _chk(self.L.phyhip_set_stream(self.id, C.c_void_p(stream_handle)))

    def synchronize(self):
        _chk(self.L.phyhip_synchronize(self.id))

    def profile(self, enable):
        _chk(self.L.phyhip_profile(self.id, int(enable)))

    def profile_read(self):
        ms = C.c_double(0); n = C.c_int(0); u = C.c_double(0)
        _chk(self.L.phyhip_profile_read(self.id, C.byref(ms), C.byref(n), C.byref(u)))
        return ms.value, n.value, u.value

    def resident_stats(self, which=0):
        """(evaluations served by the resident workgroups, their launches, unanswered commands, evaluations launched instead)
        of the dLk evaluator; resident_stats(1): of the short-evaluation one; resident_stats(2): of the large-grid one"""
        if which == 2:  # the large-grid evaluator (phyhip_big.hpp)
            big = (C.c_longlong * 4)()
            _chk(self.L.phyhip_get_big_resident_stats(self.id, big))
            return tuple(int(v) for v in big)
        out = (C.c_longlong * 8)()
        _chk(self.L.phyhip_get_resident_stats(self.id, out))
        return tuple(int(v) for v in out[4 * which:4 * which + 4])

    def set_virtual_buffers(self, min_operations):
        """phyhip_set_virtual_buffers: traversal launches of at least this many operations leave tip x tip results virtual
        (0: never, and what is virtual is stored)"""
        _chk(self.L.phyhip_set_virtual_buffers(self.id, int(min_operations)))

    def virtual_stats(self):
        """(buffers virtual now, stores skipped, non-storing re-issues, storing re-issues)"""
        out = (C.c_longlong * 4)()
        _chk(self.L.phyhip_get_virtual_stats(self.id, out))
        return tuple(int(v) for v in out)

    def deferred_stats(self):
        """(buffers deferred now, stores deferred, definitions stored on demand, definitions dropped)"""
        out = (C.c_longlong * 4)()
        _chk(self.L.phyhip_get_deferred_stats(self.id, out))
        return tuple(int(v) for v in out)

    def set_chained_buffers(self, min_operations):
        """phyhip_set_chained_buffers: one-sided traversal launches of at least this many operations leave forwarded results whose
        children are unstored themselves unstored as well (0: never; what is chained stays so until something needs it)"""
        _chk(self.L.phyhip_set_chained_buffers(self.id, int(min_operations)))

    def chained_stats(self):
        """(buffers chained now, stores left out, definitions stored on demand, definitions dropped)"""
        out = (C.c_longlong * 4)()
        _chk(self.L.phyhip_get_chained_stats(self.id, out))
        return tuple(int(v) for v in out)

    def record_stats(self):
        """phyhip_get_record_stats: (compact lists built, launches served from a device slot, then per child position five counts:
        tip, in-step, forwarded k-1, forwarded k-2, loaded)"""
        out = (C.c_longlong * 12)()
        _chk(self.L.phyhip_get_record_stats(self.id, out))
        return tuple(int(v) for v in out)

    def step_kind_stats(self):
        """phyhip_get_step_kind_stats: ((kinds 0-7 of the even steps), (of the odd steps)) over the compact lists built; kind 0 is
        the generic step, 1 tip x forwarded k-1, 2 forwarded k-1 x tip, 3 in-step x forwarded k-1, 4 forwarded k-1 x in-step,
        5 in-step x tip, 6 tip x in-step"""
        out = (C.c_longlong * 16)()
        _chk(self.L.phyhip_get_step_kind_stats(self.id, out))
        return tuple(int(v) for v in out[:8]), tuple(int(v) for v in out[8:])

    def profile_read_eigen(self):
        """(ms, launches) of eigen_lr_kernel and of dlk_kernel since profile(1)"""
        a = C.c_double(0); an = C.c_int(0); b = C.c_double(0); bn = C.c_int(0)
        _chk(self.L.phyhip_profile_read_eigen(self.id, C.byref(a), C.byref(an), C.byref(b), C.byref(bn)))
        return (a.value, an.value), (b.value, bn.value)

    def profile_read_collective(self):
        """(ms, evaluations, ranks) of the collective path (local sum, all-reduce, publish) since profile(1)"""
        ms = C.c_double(0); n = C.c_int(0); r = C.c_int(0)
        _chk(self.L.phyhip_profile_read_collective(self.id, C.byref(ms), C.byref(n), C.byref(r)))
        return ms.value, n.value, r.value

    def profile_read_kernel(self):
        """name of the traversal kernel of the last profiled launch (template arguments included)"""
        buf = C.create_string_buffer(128)
        _chk(self.L.phyhip_profile_read_kernel(self.id, buf, 128))
        return buf.value.decode()

    def profile_read_traffic(self):
        r = C.c_double(0); w = C.c_double(0)
        _chk(self.L.phyhip_profile_read_traffic(self.id, C.byref(r), C.byref(w)))
        return r.value, w.value


def mixture_log_likelihood(instance_ids, parents, children, matrices, proba, r_mat_weight, e_frq_weight, r_sum, e_sum, sum_probas):
    """phyhip_calculate_mixture_log_likelihood: MIXT_Lk over class instances (one category each)."""
    L = load()
    n = len(instance_ids)
    ia = lambda v: (C.c_int * n)(*[int(x) for x in v])
    da = lambda v: (C.c_double * n)(*[float(x) for x in v])
    out = C.c_double(0.0)
    _chk(L.phyhip_calculate_mixture_log_likelihood(ia(instance_ids), n, ia(parents), ia(children), ia(matrices), da(proba),
                                                   da(r_mat_weight), da(e_frq_weight), C.c_double(r_sum), C.c_double(e_sum),
                                                   C.c_double(sum_probas), C.byref(out)))
    return out.value


def mixture_regraft_log_likelihoods(instance_ids, eigen_indices, candidates, proba, r_mat_weight, e_frq_weight, r_sum, e_sum, sum_probas,
                                    keep=-1, with_warnings=False):
    """phyhip_calculate_mixture_regraft_log_likelihoods: the candidates of Instance.regraft_log_likelihoods over the class instances of
    a mixture (one category each) in one device call, combined as MIXT_Lk combines them.  eigen_indices: the eigen system of each
    class (None: 0 everywhere).  Returns the log-likelihoods [K] (and the per-candidate warnings with with_warnings)."""
    L = load()
    n = len(instance_ids)
    ia = lambda v: (C.c_int * max(1, len(v)))(*[int(x) for x in v])
    da = lambda v: (C.c_double * max(1, len(v)))(*[float(x) for x in v])
    cand = list(candidates)
    arr = (RegraftCandidate * max(1, len(cand)))()
    for k, (c1, c2, sub, flags, l1, l2, l3) in enumerate(cand):
        arr[k] = RegraftCandidate(int(c1), int(c2), int(sub), int(flags), float(l1), float(l2), float(l3))
    out = np.zeros(len(cand)); w = np.zeros(len(cand), dtype=np.int32)
    _chk(L.phyhip_calculate_mixture_regraft_log_likelihoods(ia(instance_ids), n, ia([0] * n if eigen_indices is None else eigen_indices), arr,
                                                            len(cand), int(keep), da(proba), da(r_mat_weight), da(e_frq_weight),
                                                            C.c_double(r_sum), C.c_double(e_sum), C.c_double(sum_probas), _ptr(out), _ptr(w)))
    return (out, w) if with_warnings else out


def mixture_log_likelihood_classes(instance_ids, parents, children, matrices, proba, r_mat_weight, e_frq_weight, r_sum, e_sum, sum_probas):
    """phyhip_calculate_mixture_log_likelihood with class-axis instances among the entries: the per-class tables are longer than
    the instance list (an entry stands for its C classes)."""
    L = load()
    n = len(instance_ids)
    ia = lambda v: (C.c_int * len(v))(*[int(x) for x in v])
    da = lambda v: (C.c_double * len(v))(*[float(x) for x in v])
    out = C.c_double(0.0)
    _chk(L.phyhip_calculate_mixture_log_likelihood(ia(instance_ids), n, ia(parents), ia(children), ia(matrices), da(proba),
                                                   da(r_mat_weight), da(e_frq_weight), C.c_double(r_sum), C.c_double(e_sum),
                                                   C.c_double(sum_probas), C.byref(out)))
    return out.value


def mixture_eigen_lnl_dlnl(instance_ids, lefts, rights, l, proba, r_mat_weight, e_frq_weight, r_sum, e_sum, sum_probas):
    """phyhip_calculate_mixture_eigen_lnl_dlnl: MIXT_dLk over class instances; returns (clamped l, lnL, dlnL)."""
    L = load()
    n = len(instance_ids)
    ia = lambda v: (C.c_int * n)(*[int(x) for x in v])
    da = lambda v: (C.c_double * n)(*[float(x) for x in v])
    lv, lnl, dlnl = C.c_double(l), C.c_double(0.0), C.c_double(0.0)
    _chk(L.phyhip_calculate_mixture_eigen_lnl_dlnl(ia(instance_ids), n, ia(lefts), ia(rights), C.byref(lv), da(proba),
                                                   da(r_mat_weight), da(e_frq_weight), C.c_double(r_sum), C.c_double(e_sum),
                                                   C.c_double(sum_probas), C.byref(lnl), C.byref(dlnl)))
    return lv.value, lnl.value, dlnl.value
