"""Python handle on the C host layer (libphyhip_lk.so, include/phyhip_lk.h).

The host side of the likelihood surface -- `Lk`, `dLk`, `Update_Partial_Lk`, `Post_Order_Lk`, ... with
the reference's names and argument meaning (src/lk.h:27-159) -- is plain C in
phyml_amd/csrc/host/phl_lk.c, as in the reference.  This module only mirrors its structs with ctypes
so that the parity tests and bench.py can drive it; no arithmetic and no tree logic lives here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LK_LIB_PATH = os.path.join(capi.LIB_DIR, "libphyhip_lk.so")


class t_node(C.Structure):
    pass


class t_edge(C.Structure):
    pass


t_node._fields_ = [("v", C.POINTER(t_node) * 3), ("b", C.POINTER(t_edge) * 3), ("num", C.c_int), ("tax", C.c_int)]
t_edge._fields_ = [("left", C.POINTER(t_node)), ("rght", C.POINTER(t_node)), ("num", C.c_int), ("l", C.c_double),
                   ("Pij_rr_idx", C.c_int), ("p_lk_left_idx", C.c_int), ("p_lk_rght_idx", C.c_int),
                   ("p_lk_tip_idx", C.c_int), ("update_partial_lk_left", C.c_short),
                   ("update_partial_lk_rght", C.c_short), ("Pij_rr", C.POINTER(C.c_double))]


class t_mod(C.Structure):
    _fields_ = [("ns", C.c_int), ("n_catg", C.c_int), ("pi", C.POINTER(C.c_double)),
                ("gamma_rr", C.POINTER(C.c_double)), ("gamma_r_proba", C.POINTER(C.c_double)),
                ("e_val", C.POINTER(C.c_double)), ("r_e_vect", C.POINTER(C.c_double)),
                ("l_e_vect", C.POINTER(C.c_double)), ("l_min", C.c_double), ("l_max", C.c_double),
                ("br_len_mult", C.c_double), ("invar", C.c_int), ("pinvar", C.c_double), ("use_m4mod", C.c_int)]


class t_tree(C.Structure):
    _fields_ = [("a_nodes", C.POINTER(C.POINTER(t_node))), ("a_edges", C.POINTER(C.POINTER(t_edge))),
                ("mod", C.POINTER(t_mod)), ("n_otu", C.c_int), ("n_pattern", C.c_int),
                ("wght", C.POINTER(C.c_double)), ("invar", C.POINTER(C.c_short)), ("b_inst", C.c_int),
                ("tip_root", C.c_int), ("both_sides", C.c_short), ("use_eigen_lr", C.c_short),
                ("update_eigen_lr", C.c_short), ("apply_lk_scaling", C.c_short), ("numerical_warning", C.c_short),
                ("host_pmat", C.c_short), ("c_lnL", C.c_double), ("old_lnL", C.c_double), ("c_dlnL", C.c_double),
                ("n_edges_traversed", C.c_int), ("spare_p_lk_idx", C.c_int), ("spare_Pij_idx", C.c_int),
                ("e_root", C.POINTER(t_edge)), ("do_alias_subpatt", C.c_short), ("update_alias_subpatt", C.c_short),
                ("alias_one_subpatt", C.c_void_p), ("init_len", C.c_int), ("sh_seed", C.c_ulonglong)]


class t_tree_pars(t_tree):
    """t_tree with the parsimony fields the C struct has appended behind sh_seed (a ctypes subclass lays its fields out behind the
    base's): what the host layer's trees are"""
    _fields_ = [("c_pars", C.c_int), ("best_pars", C.c_int), ("site_pars", C.POINTER(C.c_int)), ("general_pars", C.c_short),
                ("step_mat", C.POINTER(C.c_int)), ("own_step_mat", C.c_short)]


class t_mod_brlen(t_mod):
    """t_mod with the fields Br_Len_Opt reads, appended behind use_m4mod: what Make_Model_Basic allocates (LkTree.s_opt casts)"""
    _fields_ = [("min_diff_lk_local", C.c_double), ("brent_it_max", C.c_int)]


class t_tree_brlen(C.Structure):
    """... and t_tree with Br_Len_Opt's fields behind the parsimony ones: what the host layer's trees are.  One flat structure: the C
    compiler packs n_tot_bl_opt into the tail padding behind own_step_mat, where a ctypes subclass would start behind it"""
    _fields_ = t_tree._fields_ + t_tree_pars._fields_ + [
        ("n_tot_bl_opt", C.c_int), ("bl_opt_evaluations", C.c_int), ("bl_opt_status", C.c_int),
        ("bl_opt_host_chain", C.c_short), ("bl_opt_on_device", C.c_short)]


_lib = None
_errors = []


@C.CFUNCTYPE(None, C.c_char_p)
def _exit_handler(msg):
    _errors.append(msg.decode(errors="replace"))


def load():
    global _lib
    if _lib is None:
        capi.load()  # libphyhip.so first (the host layer links against it)
        if not os.path.exists(LK_LIB_PATH):
            raise capi.PhyhipError(f"{LK_LIB_PATH} not built: run __graft_entry__.build()")
        L = C.CDLL(LK_LIB_PATH)
        L.Make_Tree_From_Edges.restype = C.POINTER(t_tree_brlen)
        L.Make_Model_Basic.restype = C.POINTER(t_mod)
        for f in ("Lk", "dLk", "Br_Len_Newton", "Br_Len_Opt", "Triple_Dist", "Update_Lk_At_Given_Edge", "Get_Exact_Site_Lk", "Statistics_To_SH", "Statistics_to_RELL"):
            getattr(L, f).restype = C.c_double
        # tests must survive the reference's print-and-Exit() convention
        L.Set_Exit_Handler(_exit_handler)
        _lib = L
    return _lib


def _raise_if_error():
    if _errors:
        msg = "".join(_errors)
        _errors.clear()
        raise capi.PhyhipError(msg.strip())


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class LkTree:
    """Owns a C `t_tree` + `t_mod`.  Methods are one-line forwards to the C functions of the same name."""

    def __init__(self, n_otu, edge_left, edge_rght, edge_len, n_pattern, ns, ncatg, device=None, node_v=None,
                 node_b=None, host_pmat=False, devices=None, force_sharded=False, class_axis=False, use_m4mod=False):
        L = load()
        self.L = L
        self.n, self.P, self.S, self.C = int(n_otu), int(n_pattern), int(ns), int(ncatg)
        el = np.ascontiguousarray(edge_left, dtype=np.int32); er = np.ascontiguousarray(edge_rght, dtype=np.int32)
        ln = np.ascontiguousarray(edge_len, dtype=np.float64)
        nv = None if node_v is None else np.ascontiguousarray(node_v, dtype=np.int32)
        nb = None if node_b is None else np.ascontiguousarray(node_b, dtype=np.int32)
        self.ne = len(el)
        self.tree = L.Make_Tree_From_Edges(self.n, el.ctypes.data_as(C.c_void_p), er.ctypes.data_as(C.c_void_p), _dp(ln),
                                           None if nv is None else nv.ctypes.data_as(C.c_void_p),
                                           None if nb is None else nb.ctypes.data_as(C.c_void_p))
        self.mod = L.Make_Model_Basic(self.S, self.C)
        self.tree.contents.mod = self.mod
        self.tree.contents.host_pmat = 1 if host_pmat else 0
        self.mod.contents.use_m4mod = 1 if use_m4mod else 0  # `phyml --cov`: the reference's generic loop (PHYHIP_FLAG_GENERIC_LOOP)
        self.device = -1 if device is None else int(device)
        # multi-GPU: pattern shards over `devices` inside libphyhip.so (one RCCL all-reduce per evaluation)
        self.devices = None if devices is None else [int(x) for x in devices]
        self.force_sharded = bool(force_sharded)
        self.class_axis = bool(class_axis)  # categories = classes of a mixture (PHYHIP_FLAG_CLASS_AXIS)
        self._made = False
        self.inst = None

    # --- model / data ------------------------------------------------------------------------------
    def set_model(self, pi, gamma_rr, gamma_r_proba, e_val, r_e_vect, l_e_vect, l_min=1e-8, l_max=100.0,
                  br_len_mult=1.0, apply_lk_scaling=1, invar_model=0, pinvar=0.0):
        m = self.mod.contents
        for dst, src, n in ((m.pi, pi, self.S), (m.gamma_rr, gamma_rr, self.C), (m.gamma_r_proba, gamma_r_proba, self.C),
                            (m.e_val, e_val, self.S), (m.r_e_vect, r_e_vect, self.S * self.S),
                            (m.l_e_vect, l_e_vect, self.S * self.S)):
            a = np.ascontiguousarray(src, dtype=np.float64).ravel()
            assert a.size == n
            C.memmove(dst, a.ctypes.data, 8 * n)
        m.l_min, m.l_max, m.br_len_mult = float(l_min), float(l_max), float(br_len_mult)
        m.invar, m.pinvar = int(invar_model), float(pinvar)
        self.tree.contents.apply_lk_scaling = int(apply_lk_scaling)
        if self._made:
            self.L.Update_Model_On_Device(self.tree)
            _raise_if_error()

    def Make_Tree_For_Lk(self, wght, invar=None):
        w = np.ascontiguousarray(wght, dtype=np.float64); assert w.size == self.P
        iv = None if invar is None else np.ascontiguousarray(invar, dtype=np.int16)
        ivp = None if iv is None else iv.ctypes.data_as(C.c_void_p)
        if self.devices is not None or self.class_axis:
            devs = self.devices if self.devices is not None else ([self.device] if self.device >= 0 else [])
            dv = (C.c_int * max(1, len(devs)))(*devs)
            self.L.Make_Tree_For_Lk_On_Devices(self.tree, self.P, _dp(w), ivp, dv, len(devs),
                                               (1 if self.force_sharded else 0) | (2 if self.class_axis else 0))
        else:
            self.L.Make_Tree_For_Lk(self.tree, self.P, _dp(w), ivp, self.device)
        _raise_if_error()
        self._made = True
        self.inst = _InstanceView(self.tree.contents.b_inst, self)

    def set_tips(self, tip_partials=None, tip_states=None, tip_chars=None):
        for t in range(self.n):
            if tip_chars is not None:  # compressed sequences as characters: the host layer's own encoders (src/lk.c:26-161)
                seq = bytes(np.ascontiguousarray(tip_chars[t], dtype=np.uint8)); assert len(seq) == self.P
                self.L.Init_Partial_Lk_Tips_Chars_One_Tip(self.tree, t, C.c_char_p(seq))
            elif tip_partials is not None:
                a = np.ascontiguousarray(tip_partials[t], dtype=np.float64); assert a.size == self.P * self.S
                self.L.Init_Partial_Lk_Tips_Double_One_Tip(self.tree, t, _dp(a))
            else:
                a = np.ascontiguousarray(tip_states[t], dtype=np.int32); assert a.size == self.P
                self.L.Init_Partial_Lk_Tips_States_One_Tip(self.tree, t, a.ctypes.data_as(C.c_void_p))
            _raise_if_error()

    def close(self):
        if self.tree is not None:
            if self._made:
                self.L.Free_Tree_Lk(self.tree)
            self.L.Free_Tree(self.tree)
            self.L.Free_Model(self.mod)
            self.tree = None

    # --- accessors ---------------------------------------------------------------------------------------
    def edge(self, e):
        return self.tree.contents.a_edges[e]

    def node(self, k):
        return self.tree.contents.a_nodes[k]

    @property
    def c_lnL(self):
        return self.tree.contents.c_lnL

    @property
    def c_dlnL(self):
        return self.tree.contents.c_dlnL

    @property
    def tip_root(self):
        return self.tree.contents.tip_root

    @tip_root.setter
    def tip_root(self, v):
        self.tree.contents.tip_root = int(v)

    # --- the surface (same names as src/lk.h) ------------------------------------------------------------------
    def Lk(self, b=None):
        v = self.L.Lk(None if b is None else self.edge(b), self.tree)
        _raise_if_error()
        return v

    def Exact_Site_Lk(self, b=None):
        """Get_Exact_Site_Lk: (ordered sum, c_lnL_sorted, cur_site_lk, unscaled_site_lk_cat, fact_sum_scale) of edge b (None: the
        edge Lk(None) evaluates) as the reference's doubles; the partials on both sides of b must be current."""
        a = np.zeros(self.P); c = np.zeros(self.P); u = np.zeros((self.P, self.C)); f = np.zeros(self.P, np.int32)
        v = self.L.Get_Exact_Site_Lk(self.tree, None if b is None else self.edge(b), _dp(a), _dp(c), _dp(u),
                                     f.ctypes.data_as(C.c_void_p))
        _raise_if_error()
        return v, a, c, u, f

    def Ancestral_Probs(self, d=None):
        """Get_Ancestral_Probs(d): the marginal state posteriors [pattern][state] of internal node d; d=None:
        Get_All_Ancestral_Probs, [n_otu - 2][pattern][state], row k = node n_otu + k.  The partials on every side must be current
        and the last evaluation's per-site log-likelihoods the tree's (Set_Both_Sides(True); Lk(None))."""
        if d is None:
            out = np.zeros((self.n - 2, self.P, self.S))
            self.L.Get_All_Ancestral_Probs(self.tree, _dp(out))
        else:
            out = np.zeros((self.P, self.S))
            self.L.Get_Ancestral_Probs(self.tree, self.node(d), _dp(out))
        _raise_if_error()
        return out

    def ML_Dist(self, min_diff_lk_local=1e-3):
        """ML_Dist: the [n_otu][n_otu] pairwise ML distance matrix of the loaded tips under the loaded model, on the device"""
        out = np.zeros((self.n, self.n))
        self.L.ML_Dist(self.tree, C.c_double(min_diff_lk_local), _dp(out))
        _raise_if_error()
        return out

    def Set_Log_Lks_aLRT(self, k):
        """log_lks_aLRT[k] = c_lnL_sorted of the Lk(b) that has just run, kept on the device (k = 0..2)"""
        self.L.Set_Log_Lks_aLRT(self.tree, int(k)); _raise_if_error()

    def Statistics_To_SH(self, init_len=None, seed=None):
        """Statistics_To_SH: the SH-like support from the three snapshots, 10 000 replicates of init_len sites on the device
        (init_len / seed: tree->init_len / tree->sh_seed are set first when given)"""
        if init_len is not None: self.tree.contents.init_len = int(init_len)
        if seed is not None: self.tree.contents.sh_seed = int(seed)
        v = self.L.Statistics_To_SH(self.tree); _raise_if_error()
        return v

    def Statistics_to_RELL(self, init_len=None, seed=None):
        """Statistics_to_RELL (deprecated in the reference): the RELL support from the same pass"""
        if init_len is not None: self.tree.contents.init_len = int(init_len)
        if seed is not None: self.tree.contents.sh_seed = int(seed)
        v = self.L.Statistics_to_RELL(self.tree); _raise_if_error()
        return v

    # --- parsimony (same names as src/pars.h) ----------------------------------------------------------------
    def Make_Tree_For_Pars(self, general_pars=False, step_mat=None):
        """Make_Tree_For_Pars after tree->general_pars (and, given, the caller's own tree->step_mat [ns][ns]) are set; re-callable"""
        t = self.tree.contents
        t.general_pars = 1 if general_pars else 0
        if step_mat is not None:
            if t.own_step_mat:
                self.L.Free_Tree_Pars(self.tree)
            self._step_mat = np.ascontiguousarray(step_mat, dtype=np.int32); assert self._step_mat.size == self.S * self.S
            t.step_mat = self._step_mat.ctypes.data_as(C.POINTER(C.c_int))
            t.own_step_mat = 0
        self.L.Make_Tree_For_Pars(self.tree); _raise_if_error()

    def Pars(self, b=None):
        v = self.L.Pars(None if b is None else self.edge(b), self.tree); _raise_if_error()
        return v

    def Update_Partial_Pars(self, b, n):
        self.L.Update_Partial_Pars(self.tree, self.edge(b), self.node(n)); _raise_if_error()

    def Update_Pars_At_Given_Edge(self, b):
        v = self.L.Update_Pars_At_Given_Edge(self.edge(b), self.tree); _raise_if_error()
        return v

    def Get_Partial_Pars(self, b, side):
        """(ui, pars) of edge b's left (side 0) or right (1) side, or p_pars [pattern][state] in the step-matrix mode"""
        e = self.edge(b).contents
        d = e.left if side == 0 else e.rght
        ip = lambda a: a.ctypes.data_as(C.c_void_p)
        if self.tree.contents.general_pars:
            pp = np.zeros((self.P, self.S), np.int32)
            self.L.Get_Partial_Pars(self.tree, self.edge(b), d, None, None, ip(pp)); _raise_if_error()
            return pp
        ui = np.zeros(self.P, np.int32); pars = np.zeros(self.P, np.int32)
        self.L.Get_Partial_Pars(self.tree, self.edge(b), d, ip(ui), ip(pars), None); _raise_if_error()
        return ui, pars

    def Pars_Regraft_Scan(self, b_sub, d_sub, targets, keep=-1):
        """Pars_Regraft_Scan: the parsimony scores [n] of regrafting the subtree of edge b_sub on node d_sub's side onto each edge of
        `targets` -- one device call.  keep: the candidate whose vectors stay for Get_Regraft_Partial_Pars / Get_Regraft_Site_Pars.
        On an intact tree the vectors are whatever the tree holds (include/phyhip_lk.h)."""
        n = len(targets)
        tg = (C.POINTER(t_edge) * max(1, n))(*[self.edge(int(b)) for b in targets])
        out = np.zeros(n, np.int32)
        self.L.Pars_Regraft_Scan(self.tree, self.edge(int(b_sub)), self.node(int(d_sub)), n, tg, int(keep), out.ctypes.data_as(C.c_void_p))
        _raise_if_error()
        return out

    def Get_Regraft_Partial_Pars(self):
        """(ui, pars) of the kept candidate's joined vector, or p_pars [pattern][state] in the step-matrix mode"""
        ip = lambda a: a.ctypes.data_as(C.c_void_p)
        if self.tree.contents.general_pars:
            pp = np.zeros((self.P, self.S), np.int32)
            self.L.Get_Regraft_Partial_Pars(self.tree, None, None, ip(pp)); _raise_if_error()
            return pp
        ui = np.zeros(self.P, np.int32); pars = np.zeros(self.P, np.int32)
        self.L.Get_Regraft_Partial_Pars(self.tree, ip(ui), ip(pars), None); _raise_if_error()
        return ui, pars

    def Get_Regraft_Site_Pars(self):
        out = np.zeros(self.P, np.int32)
        self.L.Get_Regraft_Site_Pars(self.tree, out.ctypes.data_as(C.c_void_p)); _raise_if_error()
        return out

    @property
    def c_pars(self):
        return self.tree.contents.c_pars

    @property
    def site_pars(self):
        return np.ctypeslib.as_array(self.tree.contents.site_pars, shape=(self.P,)).copy()

    @property
    def step_mat(self):
        return np.ctypeslib.as_array(self.tree.contents.step_mat, shape=(self.S, self.S)).copy()

    def dLk(self, l, b):
        lv = C.c_double(l)
        v = self.L.dLk(C.byref(lv), self.edge(b), self.tree)
        _raise_if_error()
        return lv.value, v

    def Update_Partial_Lk(self, b, d):
        self.L.Update_Partial_Lk(self.tree, self.edge(b), self.node(d)); _raise_if_error()

    def set_root_edge(self, b):
        """Rooted input tree with the root ignored (tree->e_root; None: unrooted)."""
        self.tree.contents.e_root = self.edge(b) if b is not None else C.POINTER(t_edge)()

    def Update_Lk_At_Given_Edge(self, b):
        v = self.L.Update_Lk_At_Given_Edge(self.edge(b), self.tree); _raise_if_error()
        return v

    def Update_PMat_At_Given_Edge(self, b):
        self.L.Update_PMat_At_Given_Edge(self.edge(b), self.tree); _raise_if_error()

    def Post_Order_Lk(self, a, d):
        self.L.Post_Order_Lk(self.node(a), self.node(d), self.tree); _raise_if_error()

    def Pre_Order_Lk(self, a, d):
        self.L.Pre_Order_Lk(self.node(a), self.node(d), self.tree); _raise_if_error()

    def Update_All_Partial_Lk(self):
        self.L.Update_All_Partial_Lk(self.tree); _raise_if_error()

    def Update_Eigen_Lr(self, b):
        self.L.Update_Eigen_Lr(self.edge(b), self.tree); _raise_if_error()

    def Set_Both_Sides(self, yesno):
        self.L.Set_Both_Sides(int(bool(yesno)), self.tree)

    def Set_Use_Eigen_Lr(self, yesno):
        self.L.Set_Use_Eigen_Lr(int(bool(yesno)), self.tree)

    def Set_Update_Eigen_Lr(self, yesno):
        self.L.Set_Update_Eigen_Lr(int(bool(yesno)), self.tree)

    def Br_Len_Newton(self, b):
        lv = C.c_double(self.edge(b).contents.l)
        v = self.L.Br_Len_Newton(C.byref(lv), self.edge(b), self.tree)
        _raise_if_error()
        return lv.value, v

    def Br_Len_Opt(self, b, force_host_chain=False, l=None, force_device=False):
        """Br_Len_Opt(&b->l, b, tree) (src/optimiz.c:607): the edge's length optimised from its own value, or from `l`, which becomes
        b->l first -- the search in one device call, or (force_host_chain, and wherever the call is not built for the instance) the same
        search driving dLk() from the host.  By default the host layer drives dLk() (measured the faster route on all but one shape);
        force_device takes the device call wherever it is built.  Returns (l, lnL, dlnL, evaluations, status); `on_device` says which route the search took."""
        e = self.edge(b).contents
        if l is not None:
            e.l = float(l)
        tr = self.tree.contents
        tr.bl_opt_host_chain = 1 if force_host_chain else (2 if force_device else 0)
        lp = C.cast(C.byref(e, t_edge.l.offset), C.POINTER(C.c_double))
        v = self.L.Br_Len_Opt(lp, self.edge(b), self.tree)
        tr.bl_opt_host_chain = 0
        _raise_if_error()
        return e.l, v, tr.c_dlnL, tr.bl_opt_evaluations, tr.bl_opt_status

    def Regraft_Scan(self, b_sub, d_sub, link_is_left, l_sub, targets, l_left, l_rght):
        """Lk_Regraft_Scan: the log-likelihoods [n] of regrafting the subtree of edge b_sub on node d_sub's side, on a branch of length
        l_sub, onto each edge of `targets` cut into halves of l_left[i] / l_rght[i] -- one device call.  On an intact tree the
        vectors are whatever the tree holds (include/phyhip_lk.h)."""
        n = len(targets)
        tg = (C.POINTER(t_edge) * max(1, n))(*[self.edge(int(b)) for b in targets])
        ll = np.ascontiguousarray(l_left, dtype=np.float64); lr = np.ascontiguousarray(l_rght, dtype=np.float64)
        assert ll.size == n and lr.size == n
        out = np.zeros(n)
        self.L.Lk_Regraft_Scan(self.tree, self.edge(int(b_sub)), self.node(int(d_sub)), 1 if link_is_left else 0, C.c_double(l_sub),
                               n, tg, _dp(ll), _dp(lr), _dp(out))
        _raise_if_error()
        return out

    def Triple_Dist(self, a, force_host_chain=True, force_device=False):
        """Triple_Dist(a, tree) (src/utilities.c:7120) at node number a, driven call by call through this layer's Update_Partial_Lk and
        Br_Len_Opt (whose search takes the route the two flags name, as LkTree.Br_Len_Opt's do); changes the tree as the reference
        does.  Returns ((l0, l1, l2), c_lnL, growth of n_tot_bl_opt)."""
        tr = self.tree.contents
        tr.bl_opt_host_chain = 2 if force_device else (1 if force_host_chain else 0)
        before = tr.n_tot_bl_opt
        v = self.L.Triple_Dist(self.node(int(a)), self.tree)
        tr.bl_opt_host_chain = 0
        _raise_if_error()
        nd = self.node(int(a)).contents
        return tuple(nd.b[i].contents.l for i in range(3)), v, tr.n_tot_bl_opt - before

    def Triple_Dist_Scan(self, nodes):
        """Triple_Dist_Scan: what Triple_Dist would find at each node of `nodes`, each from the tree as it stands, in one device call;
        the tree's lengths, buffers and c_lnL are left alone (include/phyhip_lk.h).  Returns (lengths [n][3], lnL [n], status [n])."""
        n = len(nodes)
        nd = (C.POINTER(t_node) * max(1, n))(*[self.node(int(a)) for a in nodes])
        l_out = np.zeros((n, 3)); lnl = np.zeros(n); st = np.zeros(n, np.int32)
        self.L.Triple_Dist_Scan(self.tree, n, nd, _dp(l_out), _dp(lnl), st.ctypes.data_as(C.c_void_p))
        _raise_if_error()
        return l_out, lnl, st

    @property
    def s_opt(self):
        """the model's min_diff_lk_local / brent_it_max (mod->s_opt in the reference), readable and writable"""
        return C.cast(self.mod, C.POINTER(t_mod_brlen)).contents

    @property
    def on_device(self):
        """whether the last Br_Len_Opt's search was the device call (phyhip_optimise_edge_length)"""
        return bool(self.tree.contents.bl_opt_on_device)

    @property
    def n_tot_bl_opt(self):
        return self.tree.contents.n_tot_bl_opt

    def Replay_Surface_Trace(self, trace):
        """trace: dict of equal-length arrays kind,a,b,c,d,e (int32) and x (float64); returns (out, out2)."""
        n = len(trace["kind"])
        arr = {k: np.ascontiguousarray(trace[k], dtype=np.int32) for k in ("kind", "a", "b", "c", "d", "e")}
        x = np.ascontiguousarray(trace["x"], dtype=np.float64)
        out = np.zeros(n); out2 = np.zeros(n)
        ip = lambda v: v.ctypes.data_as(C.c_void_p)
        self.L.Replay_Surface_Trace(self.tree, n, ip(arr["kind"]), ip(arr["a"]), ip(arr["b"]), ip(arr["c"]), ip(arr["d"]),
                                    ip(arr["e"]), _dp(x), _dp(out), _dp(out2))
        _raise_if_error()
        return out, out2

    @property
    def spare_p_lk_idx(self):
        return self.tree.contents.spare_p_lk_idx

    @property
    def spare_Pij_idx(self):
        return self.tree.contents.spare_Pij_idx

    def Lk_Shard_Device(self, device_ptr):
        self.L.Lk_Shard_Device(self.tree, C.c_void_p(device_ptr)); _raise_if_error()

    # --- download hooks ---------------------------------------------------------------------------------------------
    def side_buffer(self, b, side):
        e = self.edge(b).contents
        return e.p_lk_left_idx if side == 0 else e.p_lk_rght_idx

    def partials(self, b, side):
        return self.inst.get_partials(self.side_buffer(b, side))

    def scale_factors(self, b, side):
        return self.inst.get_scale_factors(self.side_buffer(b, side))


class _InstanceView(capi.Instance):
    """capi.Instance methods on an instance id that the C host layer created (no ownership)."""

    def __init__(self, inst_id, tree: LkTree):
        self.L = capi.load()
        self.id = inst_id
        self.tips, self.S, self.P, self.C = tree.n, tree.S, tree.P, tree.C
        self.nmat = tree.ne + 4
        self.details = None

    def close(self):
        self.id = None


def Mixture_Regraft_Scan(trees, proba, r_mat_weight, e_frq_weight, r_sum, e_sum, sum_probas, b_sub, d_sub, link_is_left, l_sub, targets,
                         l_left, l_rght):
    """MIXT_Lk_Regraft_Scan: LkTree.Regraft_Scan over the class trees of a mixture (`trees`: one LkTree of one category per class, the
    same topology and numbering) in one device call -- the log-likelihoods [n] MIXT_Lk would return for regrafting the subtree of edge
    b_sub on node d_sub's side onto each edge of `targets`.  Edges and nodes are numbers of the first class tree; the lengths are the
    mixture tree's (include/phyhip_lk.h)."""
    t0, K, n = trees[0], len(trees), len(targets)
    tr = (C.POINTER(t_tree_brlen) * K)(*[t.tree for t in trees])
    da = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    pr, rw, ew = da(proba), da(r_mat_weight), da(e_frq_weight)
    assert pr.size == K and rw.size == K and ew.size == K
    tg = (C.POINTER(t_edge) * max(1, n))(*[t0.edge(int(b)) for b in targets])
    ll, lr = da(l_left), da(l_rght)
    assert ll.size == n and lr.size == n
    out = np.zeros(n)
    t0.L.MIXT_Lk_Regraft_Scan(tr, K, _dp(pr), _dp(rw), _dp(ew), C.c_double(r_sum), C.c_double(e_sum), C.c_double(sum_probas),
                              t0.edge(int(b_sub)), t0.node(int(d_sub)), 1 if link_is_left else 0, C.c_double(l_sub), n, tg, _dp(ll), _dp(lr),
                              _dp(out))
    _raise_if_error()
    return out
