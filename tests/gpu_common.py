"""Helpers shared by the GPU parity tests: build a device LkTree (C host layer) from a golden dump."""
import numpy as np

import orc
from phyml_amd import lktree


def device_tree_from_golden(d, host_pmat=True, devices=None, force_sharded=False, use_m4mod=False, arith=1):
    """Device tree with the reference's own neighbour order (node_v/node_b of the dump); tips come from the
    oracle's tip encoder.  host_pmat=True: the C host layer's own PMat() + upload (bit-exact route, src/lk.c:2360);
    False: device PMat from the eigen system (src/lk.c:2344)."""
    ot = orc.tree_from_golden(d, arith=arith)
    m = ot.m
    t = lktree.LkTree(ot.n, d["edge_left"], d["edge_rght"], d["edge_len"], ot.P, m.ns, m.ncatg,
                      node_v=d["node_v"], node_b=d["node_b"], host_pmat=host_pmat, devices=devices, force_sharded=force_sharded,
                      use_m4mod=use_m4mod)
    t.tip_root = ot.tip_root
    t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, m.br_len_mult,
                int(d["apply_lk_scaling"][0]), m.invar_model, m.pinvar)
    t.Make_Tree_For_Lk(d["wght"], d["invar"])
    t.set_tips(tip_partials=ot.tip_vec)
    return t, ot


def synthetic_oracle(n_otu, P, ns, C, seed, lmin=0.02, lmax=0.3, wght=None, apply_scaling=1, ambiguous_every=0, arith=1, pinvar=None,
                     constant_every=0):
    """The oracle half of synthetic_pair (no device needed): (oracle tree, random tree, states, tip vectors, weights).
    constant_every: every constant_every-th column is made constant and unambiguous (the first taxon's simulated state in every row).
    pinvar: the +I model with that proportion; the oracle tree's `invar` is derived from the columns -- the state of a column in
    which every taxon shows the same unambiguous state, -1 elsewhere."""
    from phyml_amd import synth, workloads
    blk = dict(workloads.model_block("model_gtr_g4" if ns == 4 else "model_lg_g4"))
    rates = np.linspace(0.2, 2.2, C) if C > 1 else np.array([1.0])
    w = np.linspace(1.0, 2.0, C); w = w / w.sum()
    rates = rates / float((rates * w).sum())
    blk["ncatg"] = np.array([float(C)]); blk["gamma_rr"] = rates; blk["gamma_r_proba"] = w
    if pinvar is not None:
        blk["invar_model"] = np.array([1.0]); blk["pinvar"] = np.array([float(pinvar)])
    m = orc.Model(blk)
    tree = synth.random_tree(n_otu, seed, lmin, lmax)
    st = synth.simulate_states(tree, P, ns, seed)
    chars = synth.states_to_chars(st, ns).copy()
    if ambiguous_every:
        amb = (b"N-RY?" if ns == 4 else b"X-?BZ")
        for t in range(n_otu):
            idx = np.arange((t * 7) % ambiguous_every, P, ambiguous_every)
            chars[t, idx] = np.frombuffer(amb, dtype=np.uint8)[(idx + t) % len(amb)]
    if constant_every:
        idx = np.arange(constant_every - 1, P, constant_every)
        chars[:, idx] = synth.states_to_chars(st, ns)[0, idx]
    wg = np.ones(P) if wght is None else np.asarray(wght, dtype=np.float64)
    tv, ds, amb_ = [], [], []
    for t in range(n_otu):
        v, s, a = orc.init_tip(m.datatype, chars[t])
        tv.append(v); ds.append(s); amb_.append(a)
    invar = None
    if pinvar is not None:
        d_state, is_amb = np.array(ds), np.array(amb_)
        constant = np.all(is_amb == 0, axis=0) & np.all(d_state == d_state[0], axis=0)
        invar = np.where(constant, d_state[0], -1).astype(np.int16)
    ot = orc.OracleTree(m, n_otu, tree.edge_left, tree.edge_rght, tree.edge_len, wg, tv, ds, amb_, invar=invar, apply_scaling=apply_scaling,
                        arith=arith)
    return ot, tree, st, tv, wg


def synthetic_pair(n_otu, P, ns, C, seed, lmin=0.02, lmax=0.3, wght=None, apply_scaling=1, host_pmat=True, ambiguous_every=0,
                   devices=None, force_sharded=False, use_m4mod=False, arith=1, pinvar=None, constant_every=0):
    """Device tree + oracle tree on a seeded synthetic alignment with C rate classes (rates/weights made up,
    normalised) and the committed model block's eigen system; pinvar / constant_every: synthetic_oracle's."""
    ot, tree, st, tv, wg = synthetic_oracle(n_otu, P, ns, C, seed, lmin, lmax, wght, apply_scaling, ambiguous_every, arith, pinvar,
                                            constant_every)
    m = ot.m
    t = lktree.LkTree(n_otu, tree.edge_left, tree.edge_rght, tree.edge_len, P, ns, C, host_pmat=host_pmat, devices=devices,
                      force_sharded=force_sharded, use_m4mod=use_m4mod)
    if pinvar is None:
        t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, apply_scaling)
        t.Make_Tree_For_Lk(wg)
    else:
        t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, apply_scaling, m.invar_model,
                    m.pinvar)
        t.Make_Tree_For_Lk(wg, ot.invar)
    t.set_tips(tip_partials=tv)
    return t, ot, tree, st


def device_compute_units(device=None):
    """phyhip_instance_details::computeUnits of the device a tree is made on.  The C host layer keeps the details of the instance
    it creates to itself (t.inst.details is None), so a throw-away instance of the same device reports them."""
    from phyml_amd import capi
    inst = capi.Instance(4, 10, 4, 16, 5, 4, device=device)
    try:
        return int(inst.details.computeUnits)
    finally:
        inst.close()


def assert_device_state_is_the_oracles(t, ot, buffer_of=None, what=None):
    """What a call sequence left in device memory against the oracle tree that followed it: every transition matrix of the tree
    and every partial vector and scale vector of the tree's own buffers, bit for bit (patterns of weight zero excepted, as
    everywhere: the reference skips them).  buffer_of: {(edge, side): device buffer index} where the caller addressed the buffers
    itself (a replayed stream); else the host layer's own indices."""
    for e in range(ot.ne):
        assert np.array_equal(t.inst.get_transition_matrix(e), ot.pm[e]), (what, "matrix", e)
    w = ot.wght > 0
    for (e, side), p in ot.plk.items():
        idx = t.side_buffer(e, side) if buffer_of is None else buffer_of[(e, side)]
        assert np.array_equal(t.inst.get_partials(idx)[w], p[w]), (what, "partials", e, side)
        assert np.array_equal(t.inst.get_scale_factors(idx)[w], ot.scale[(e, side)][w]), (what, "scale", e, side)
