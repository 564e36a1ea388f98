/*
 * phyhip_lk.h -- host-side mirror (plain C) of PhyML's likelihood surface, implemented on the phyhip
 * C ABI (include/phyhip.h).  This is what spr.c / optimiz.c call in the reference (src/lk.h:27-159);
 * names, argument order and side effects follow the reference so that a caller written against lk.h
 * (or a parity test) reads the same:
 *
 *   Lk(b,tree)                      src/lk.c:443     full (b == NULL) or single-edge log-likelihood -> tree->c_lnL
 *   dLk(&l,b,tree)                  src/lk.c:655     lnL and dlnL/dl in the eigen basis -> tree->c_lnL, tree->c_dlnL
 *   Update_Partial_Lk(tree,b,d)     src/lk.c:1282    one edge-side partial vector (queued on the device)
 *   Update_PMat_At_Given_Edge(b,t)  src/lk.c:2238    transition matrices of one edge
 *   Post_Order_Lk / Pre_Order_Lk    src/lk.c:282/357 traversals issuing Update_Partial_Lk
 *   Update_All_Partial_Lk           src/lk.c:401
 *   Update_Partial_Lk_Along_A_Path  src/lk.c:2379
 *   Update_Lk_At_Given_Edge(b,tree) src/lk.c:2478    both sides of b refreshed, then Lk(b)
 *   Update_Eigen_Lr(b,tree)         src/lk.c:1038
 *   Set_Both_Sides / Set_Use_Eigen_Lr / Set_Update_Eigen_Lr   src/utilities.c:11614-11640
 *   Make_Tree_For_Lk / Free_Tree_Lk src/make.c:17 / src/free.c:387   (device instance instead of the host slab)
 *   Br_Len_Opt(&l,b,tree)           src/optimiz.c:607 one edge's length optimised: Lk(b) with update_eigen_lr, Br_Len_Spline
 *                                   (src/optimiz.c:2244) driving dLk() from the host or, where the caller asks for it, in ONE
 *                                   device call (phyhip_optimise_edge_length): the same steps; then the matrix refresh
 *   Br_Len_Newton(&l,b,tree)        NOT a reference function: a harness that drives the surface the way the caller
 *                                   Br_Len_Opt (src/optimiz.c:607-663) does -- Lk(b) with update_eigen_lr, then dLk alone,
 *                                   then the matrix refresh -- with a safeguarded Newton search on dlnL in place of the
 *                                   reference's Br_Len_Spline (src/optimiz.c:2244); optimiz.c itself stays a caller
 *
 * The structs are this repo's own minimal versions of t_tree/t_edge/t_node/t_mod: only the fields the
 * hot path reads, with the reference's field names (src/utilities.h:640-1010).  Unrooted trees, and rooted
 * input trees the way the `phyml` program evaluates them (root ignored: tree->e_root).  Errors follow the reference's
 * convention: message on stderr, then Exit() (src/utilities.c:1105) -- replaceable via Set_Exit_Handler.
 */
#ifndef PHYHIP_LK_H
#define PHYHIP_LK_H

#ifdef __cplusplus
extern "C" {
#endif

#define YES 1
#define NO 0
typedef double phydbl; /* src/utilities.h:462 */

struct __Edge;
typedef struct __Node
{
  struct __Node *v[3]; /* neighbours (NULL beyond the first for a tip) */
  struct __Edge *b[3]; /* b[i] connects this node to v[i] */
  int            num;
  int            tax;  /* 1: tip */
} t_node;

typedef struct __Edge
{
  t_node *left, *rght; /* a tip is always on the right (src/make.c:418-423) */
  int     num;
  phydbl  l;           /* b->l->v */
  /* device buffer indices: the fields the BEAGLE seam adds to t_edge (src/utilities.h:746-763) */
  int     Pij_rr_idx;
  int     p_lk_left_idx, p_lk_rght_idx, p_lk_tip_idx;
  short   update_partial_lk_left, update_partial_lk_rght; /* src/utilities.h:826-827 */
  phydbl *Pij_rr;      /* host copy [C][S][S], valid when tree->host_pmat == YES */
} t_edge;

typedef struct __Model
{
  int     ns, n_catg;            /* mod->ns, mod->ras->n_catg */
  phydbl *pi;                    /* mod->e_frq->pi->v */
  phydbl *gamma_rr;              /* mod->ras->gamma_rr->v */
  phydbl *gamma_r_proba;         /* mod->ras->gamma_r_proba->v */
  phydbl *e_val, *r_e_vect, *l_e_vect; /* mod->eigen */
  phydbl  l_min, l_max;          /* src/init.c:711-714 */
  phydbl  br_len_mult;
  int     invar;                 /* mod->ras->invar */
  phydbl  pinvar;
  int     use_m4mod;             /* mod->use_m4mod (`phyml --cov`, src/cl.c:753-757): Update_Partial_Lk sends the data through the
                                    generic loop instead of the SIMD kernels, src/lk.c:1303-1324 -- the device instance is then
                                    created with PHYHIP_FLAG_GENERIC_LOOP (that loop's arithmetic) */
  /* Br_Len_Opt (appended, every offset above stays what it was; Make_Model_Basic sets the reference's defaults, src/init.c:760,770) */
  phydbl  min_diff_lk_local;     /* mod->s_opt->min_diff_lk_local: 1.E-03 */
  int     brent_it_max;          /* mod->s_opt->brent_it_max: BRENT_IT_MAX */
} t_mod;

typedef struct __Tree
{
  t_node **a_nodes; /* [2n-2], tips first */
  t_edge **a_edges; /* [2n-3] */
  t_mod   *mod;
  int      n_otu;
  int      n_pattern;      /* tree->data->n_pattern */
  phydbl  *wght;           /* tree->data->wght */
  short   *invar;          /* tree->data->invar */
  int      b_inst;         /* device instance id (tree->b_inst, src/utilities.h:999-1001) */
  int      tip_root;
  short    both_sides, use_eigen_lr, update_eigen_lr, apply_lk_scaling, numerical_warning;
  short    host_pmat;      /* YES: PMat() on the host + upload (src/lk.c:2315,2360); NO: device PMat (src/lk.c:2344) */
  phydbl   c_lnL, old_lnL, c_dlnL;
  int      n_edges_traversed; /* counter like src/utilities.h:1018 */
  int      spare_p_lk_idx;    /* first of PHL_N_SPARE spare partials buffers (extra SPR edges, src/make.c:750) */
  int      spare_Pij_idx;     /* first of PHL_N_SPARE spare transition-matrix buffers */
  t_edge  *e_root;            /* rooted input tree with the root ignored (tree->n_root != NULL, ignore_root == YES, the only
                                 rooted form the `phyml` program evaluates): the edge the root sits on, else NULL.  The
                                 ignore_root == NO special cases of src/lk.c:2988-3146 are not built: the reference's own AVX
                                 path cannot run them (oracle/probe_rooted.sh) */
  /* `phyml --alias_subpatt` (src/cl.c:502, off by default src/init.c:624): Update_Partial_Lk calls Alias_One_Subpatt on the
     node opposite d before anything else (src/lk.c:1294-1296), tips included.  That function only maintains the host
     application's patt_id / p_lk_loc arrays (src/utilities.c:13547-13666); no likelihood function of the reference reads them
     (they are written at src/lk.c:2501-2513 and in Alias_One_Subpatt, nowhere indexed else), so the option changes no number
     of this path.  The gate is mirrored, the bookkeeping stays the application's: its own function goes here. */
  short    do_alias_subpatt, update_alias_subpatt; /* tree->io->do_alias_subpatt, tree->update_alias_subpatt */
  void   (*alias_one_subpatt)(struct __Node *a, struct __Node *d, struct __Tree *tree);
  int      init_len;          /* tree->data->init_len: sites of the alignment before compaction (Make_Tree_For_Lk sets the rounded
                                 sum of the weights; a caller whose weights are not counts sets its own) */
  unsigned long long sh_seed; /* seed of the draws of Statistics_To_SH / Statistics_to_RELL (the reference's are rand()'s; 0 at first; the
                                 caller changes it per edge for independent draws) */
  /* parsimony (src/pars.c; Make_Tree_For_Pars): appended, every offset above stays what it was */
  int      c_pars, best_pars; /* tree->c_pars, tree->best_pars */
  int     *site_pars;         /* tree->site_pars [n_pattern], filled by Pars */
  short    general_pars;      /* mod->s_opt->general_pars (`phyml --pars`): the step matrix instead of Fitch's sets */
  int     *step_mat;          /* tree->step_mat [ns][ns], row = parent state: Get_Step_Mat's for 4 states and 0/1 otherwise, or the caller's
                                 own, set before Make_Tree_For_Pars (amino acids: the reference's table is PhyML's to pass in) */
  short    own_step_mat;      /* step_mat was allocated by Get_Step_Mat (Free_Tree_Pars frees it) */
  /* Br_Len_Opt (src/optimiz.c:607): appended, every offset above stays what it was */
  int      n_tot_bl_opt;      /* tree->n_tot_bl_opt: grows by one per step of Br_Len_Spline, as in the reference (the evaluations after
                                 the first, plus one where a bracket walk leaves [l_min, l_max] before its probe) */
  int      bl_opt_evaluations, bl_opt_status; /* of the last Br_Len_Opt: dLk evaluations taken; phyhip_optimise_edge_length's status, or 8: lk_end < lk_begin - tol */
  short    bl_opt_host_chain;  /* the route of Br_Len_Opt's search.  NO and YES: dLk() driven from the host, one round trip per probe -- the default,
                                 measured the faster route on all but one shape (profiles/brlen_opt.md); 2: the device call wherever it
                                 is built, the host-driven steps where it is not (the search is the same on both routes, probe by probe) */
  short    bl_opt_on_device;   /* the last Br_Len_Opt's search was the device call */
} t_tree;

#define PHL_N_SPARE 4
#define BRENT_IT_MAX 1000 /* src/utilities.h:337 */

/* ---- construction ------------------------------------------------------------------------------ */

/* Topology from edge arrays (left/right node numbers, tips 0..n-1).  neighbour_v/neighbour_b may be NULL
   (neighbour order = edge order) or give the reference's own v[]/b[] order as [2n-2][3] node / edge numbers. */
t_tree *Make_Tree_From_Edges(int n_otu, const int *edge_left, const int *edge_rght, const phydbl *edge_len,
                             const int *neighbour_v, const int *neighbour_b);
t_mod  *Make_Model_Basic(int ns, int n_catg);
void    Free_Model(t_mod *mod);
void    Free_Tree(t_tree *tree);

/* Allocates the device instance (one partials buffer per internal edge side, one matrix per edge), uploads
   weights, +I data and the model.  device < 0: default device. */
void Make_Tree_For_Lk(t_tree *tree, int n_pattern, const phydbl *wght, const short *invar, int device);
/* the multi-GPU form: pattern shards over `devices` (see phyhip_create_instance), one RCCL all-reduce per Lk()/dLk() */
void Make_Tree_For_Lk_On_Devices(t_tree *tree, int n_pattern, const phydbl *wght, const short *invar, const int *devices,
                                 int n_devices, int flags /* 1: sharded even for one device; 2: class axis */);
void Free_Tree_Lk(t_tree *tree);
/* tip data: 0/1 tip vector [pattern][state] (a_nodes[i]->b[0]->p_lk_tip_r) or compact states */
void Init_Partial_Lk_Tips_Double_One_Tip(t_tree *tree, int tax_id, const phydbl *p_lk_tip);
void Init_Partial_Lk_Tips_States_One_Tip(t_tree *tree, int tax_id, const int *states);
/* character encoders (src/lk.c:26-69, 122-161): one alignment character -> ns 0/1 entries at p_lk[pos..]; and a whole
   compressed sequence (n_pattern characters) of one taxon, encoded and uploaded (src/lk.c:2060-2118) */
void Init_Tips_At_One_Site_Nucleotides_Float(char state, int pos, phydbl *p_lk);
void Init_Tips_At_One_Site_AA_Float(char aa, int pos, phydbl *p_lk);
void Init_Partial_Lk_Tips_Chars_One_Tip(t_tree *tree, int tax_id, const char *seq);
/* push model changes: update_beagle_ras / _efrqs / _eigen of the seam (src/beagle_utils.c:273-395) */
void Update_Model_On_Device(t_tree *tree);

/* ---- the surface ----------------------------------------------------------------------------------- */
phydbl Lk(t_edge *b, t_tree *tree);
phydbl dLk(phydbl *l, t_edge *b, t_tree *tree);
void   Update_Partial_Lk(t_tree *tree, t_edge *b, t_node *d);
void   Update_PMat_At_Given_Edge(t_edge *b_fcus, t_tree *tree);
void   Post_Order_Lk(t_node *a, t_node *d, t_tree *tree);
void   Pre_Order_Lk(t_node *a, t_node *d, t_tree *tree);
void   Update_All_Partial_Lk(t_tree *tree);
void   Update_Partial_Lk_Along_A_Path(t_node **path, int path_length, t_tree *tree);
phydbl Update_Lk_At_Given_Edge(t_edge *b_fcus, t_tree *tree); /* src/lk.c:2478-2484 */
void   Update_Eigen_Lr(t_edge *b, t_tree *tree);
void   Set_Both_Sides(int yesno, t_tree *tree);
void   Set_Use_Eigen_Lr(int yesno, t_tree *tree);
void   Set_Update_Eigen_Lr(int yesno, t_tree *tree);
/* Br_Len_Opt, src/optimiz.c:607-663: Set_Update_Eigen_Lr(YES) / Set_Use_Eigen_Lr(NO), lk_begin = Lk(b), the flags swapped, the search,
   Update_PMat_At_Given_Edge(b), both flags NO, then the decrease check of :656-661 through the exit handler.  The search is the
   step function of phyml_amd/csrc/phyhip_brlen_step.h driving dLk(): every evaluation on the device, one round trip per probe.
   With tree->bl_opt_host_chain = 2 it is phyhip_optimise_edge_length instead -- the same steps inside one kernel -- wherever that
   call is built (not: sharded, class-axis and generic-loop instances, more patterns than it serves); measured, that route is the
   faster one only on small nucleotide alignments with many long searches (profiles/brlen_opt.md), so it is not the default.
   *l, b->l, tree->c_lnL, tree->c_dlnL, tree->numerical_warning and tree->n_tot_bl_opt end as the reference leaves them; where the
   reference stops the program (statuses 3-7) the exit handler runs with its wording.  Optimize_Br_Len_Serie and MIXT_Br_Len_Opt
   stay with the caller. */
phydbl Br_Len_Opt(phydbl *l, t_edge *b, t_tree *tree);
phydbl Br_Len_Newton(phydbl *l, t_edge *b, t_tree *tree);
/* Triple_Dist, src/utilities.c:7120-7146: the matrices of a->b[1] and a->b[2], then for each of the node's three edges
   Update_Partial_Lk(tree, a->b[i], a) and Br_Len_Opt(&a->b[i]->l, a->b[i], tree), then the partials of b[1] and b[0] once more --
   driven through the functions above, one round trip per call (the per-candidate route, and the one to take wherever
   phyhip_optimise_triples refuses).  Changes the tree exactly as the reference does: the three lengths and matrices, the node's three
   partial vectors, c_lnL, c_dlnL, n_tot_bl_opt.  Where a Br_Len_Opt fails (tree->bl_opt_status 3..8: the reference's program
   ends there) and the exit handler returns, Triple_Dist returns at once: the later edges are not searched.  A tip: UNLIKELY. */
phydbl Triple_Dist(t_node *a, t_tree *tree);
/* What Triple_Dist would find at each of n internal nodes, in ONE device call (phyhip_optimise_triples): the three outer vectors of
   a[k] and their flags are resolved as Update_Partial_Lk / Lk resolve them, the start lengths are the edges' own.  l_out[k]: the three
   lengths Triple_Dist would leave on a[k]->b[0..2]; lnL[k]: its return value; status[k]: 0, or the status (3..8, include/phyhip.h)
   of the search at which the reference would have stopped the program (the lengths of that node's later edges are then their
   starts).  Any of the three may be NULL.  Updates queued before the call are seen.  The nodes are evaluated INDEPENDENTLY, each
   from the tree as it stands: the tree's lengths, matrices, partial vectors, c_lnL and c_dlnL are left alone -- a caller that
   accepts node k's result sets the lengths and runs the updates itself.  tree->n_tot_bl_opt grows by Br_Len_Opt's rule over every
   search that ran.  Batching is the caller's, and so is the bail-out of Evaluate_List_Of_Regraft_Pos_Triple (src/spr.c:1139-1376)
   at the first improving move: every node of the list is evaluated, the caller ignores the results behind that index.  Where
   the device call is not built (include/phyhip.h) the exit handler runs; the caller then takes Triple_Dist node by node. */
void Triple_Dist_Scan(t_tree *tree, int n, t_node **a, phydbl (*l_out)[3], phydbl *lnL, int *status);
/* The regraft scan of one pruned subtree in ONE device call (phyhip_calculate_regraft_log_likelihoods): what Test_One_Spr_Target
   (src/spr.c:590-760) computes target by target -- the matrices of the two halves of the target edge and of b_arrow,
   Update_Partial_Lk(b_arrow, n_link), Lk(b_arrow) -- for n target edges at once.  The subtree is the vector of b_sub on d_sub's
   side (d_sub a tip: its tip vector) and hangs on a branch of length l_sub; candidate i joins the two side vectors of b_target[i]
   through l_left[i] (the half on b_target[i]->left's side) and l_rght[i] (the right side is the tip where rght->tax); buffer
   indices are resolved as Update_Partial_Lk / Lk resolve them.  link_is_left: n_link is b_arrow->left, so the joined vector is
   Lk's left operand and the subtree the right one; NO: the subtree is the left operand (it must then be an internal node's vector).
   lnL[i]: what Lk(b_arrow) would return for candidate i.  Updates queued with Update_Partial_Lk before the call (the path updates
   of Test_One_Spr_Target_Recur, src/spr.c:543) are seen.  tree->c_lnL, every partial vector, the matrices of the edges and the
   per-site outputs are left alone.
   This layer has no Prune_Subtree / Graft_Subtree: on an INTACT tree the vectors are whatever the tree holds -- the side vectors of a
   target edge still contain the subtree, so the numbers are those of the call sequence, not of a legal SPR move; a caller that has
   pruned (or a recorded stream of a real search, tests/test_gpu_regraft.py) gets the search's candidates. */
void Lk_Regraft_Scan(t_tree *tree, t_edge *b_sub, t_node *d_sub, int link_is_left, phydbl l_sub,
                     int n, t_edge *const *b_target, const phydbl *l_left, const phydbl *l_rght, phydbl *lnL);
/* The same scan on a mixture tree, where Lk(b_arrow) dispatches to MIXT_Lk and Update_Partial_Lk to MIXT_Update_Partial_Lk: ONE device
   call over all class trees (phyhip_calculate_mixture_regraft_log_likelihoods).  class_trees[n_classes] are the class trees (one
   category each, as the mixture evaluations take them); class_proba / r_mat_weight / e_frq_weight [n_classes] and the three sums are
   MIXT_Lk's coefficients (src/mixt.c:1048-1053).  b_sub, d_sub and b_target[i] are edges and nodes of the FIRST class tree: indices are
   resolved there as Lk_Regraft_Scan resolves them -- the class trees share the numbering -- and every class tree's instance is
   passed.  l_sub, l_left[i], l_rght[i] are the mixture tree's lengths: each class applies its own rate, br_len_mult and clamp.
   lnL[i]: what MIXT_Lk(b_arrow) would return for candidate i.  Every class tree's c_lnL is left alone.  This layer has no mixture tree
   type: the caller holds the list of class trees. */
void MIXT_Lk_Regraft_Scan(t_tree *const *class_trees, int n_classes, const phydbl *class_proba, const phydbl *r_mat_weight,
                          const phydbl *e_frq_weight, phydbl r_mat_weight_sum, phydbl e_frq_weight_sum, phydbl sum_probas,
                          t_edge *b_sub, t_node *d_sub, int link_is_left, phydbl l_sub,
                          int n, t_edge *const *b_target, const phydbl *l_left, const phydbl *l_rght, phydbl *lnL);
/* host P-matrix (src/models.c:257-326, 353-373) -- used when tree->host_pmat == YES */
void   PMat(phydbl l, const t_mod *mod, int pos, phydbl *Pij);

/* sharded evaluation: same as Lk(NULL,tree) but the shard's lnL is left in device memory (no sync) */
void   Lk_Shard_Device(t_tree *tree, double *device_out);

/* Caller-side counterpart for tree search: replays a recorded stream of surface calls
   -- the calls spr.c / optimiz.c make through Update_PMat_At_Given_Edge, Update_Partial_Lk, Lk(b), Update_Eigen_Lr
   and dLk (src/spr.c:543,643-646; src/optimiz.c:622-632) -- at buffer-index level, in one C loop, and records the
   scalar every call returned.  Streams recorded from real PhyML searches (oracle/trace_driver.c) use the same
   records with buffer ids in order of first appearance.  kind[i]: */
#define PHL_REC_SET_PMAT 0 /* a = matrix index, x = edge length                               */
#define PHL_REC_UPDATE   1 /* a = dest, b = child1, c = matrix1, d = child2, e = matrix2       */
#define PHL_REC_EDGE_LNL 2 /* a = left buffer, b = right buffer or tip, c = matrix -> out = lnL */
#define PHL_REC_EIGEN_LR 3 /* a = left, b = right                                              */
#define PHL_REC_DLK      4 /* x = length -> out = lnL, out2 = dlnL                             */
#define PHL_REC_EIGEN_LNL 5 /* x = length -> out = lnL: Lk(b) in the eigen basis (src/lk.c:592-603) */
void Replay_Surface_Trace(t_tree *tree, int n_rec, const int *kind, const int *a, const int *b, const int *c, const int *d,
                          const int *e, const phydbl *x, phydbl *out, phydbl *out2);

/* download hooks for host readers (ancestral.c, cv.c, io.c) */
void Get_Partial_Lk(t_tree *tree, t_edge *b, t_node *d, phydbl *p_lk, int *sum_scale);
void Get_Site_Lk(t_tree *tree, phydbl *c_lnL_sorted, phydbl *cur_site_lk, phydbl *unscaled_site_lk_cat, int *fact_sum_scale);
/* The same arrays for edge b as the reference's doubles, bit for bit (phyhip_calculate_edge_site_outputs_exact): what aLRT,
   --print_site_lnl and cv.c read.  b == NULL: the edge Lk(NULL) evaluates (e_root, else a_nodes[tip_root]->b[0]) -- no traversal:
   as in the reference the partials on both sides of b must be current.  Returns the ordered sum of weight x c_lnL_sorted;
   tree->c_lnL and the outputs Get_Site_Lk returns are left alone.  Any pointer may be NULL. */
phydbl Get_Exact_Site_Lk(t_tree *tree, t_edge *b, phydbl *c_lnL_sorted, phydbl *cur_site_lk, phydbl *unscaled_site_lk_cat,
                         int *fact_sum_scale);

/* The marginal posterior of every state at internal node d, per pattern (phyhip_calculate_node_state_posteriors): the site loop of
   Ancestral_Sequences_One_Node (src/ancestral.c:609-901) on the device.  The three (partial vector, matrix) pairs are resolved as
   there (src/ancestral.c:661-706: v_k == b_k->left ? left : rght; a tip is its tip index).  As in the reference (src/main.c:281-288)
   the caller has run Set_Both_Sides(YES); Lk(NULL): every partial is current and the per-site log-likelihoods on the device are the
   tree's.  probs: [n_pattern][ns].  Afterwards the reference's check (src/ancestral.c:878-885): a weighted pattern whose
   probabilities are not within 0.01 of summing to 1 goes through the exit handler.  No bit parity with the reference's binary is
   claimed (include/phyhip.h).  Not built: rooted trees (tree->e_root) and mixture trees; MPEE_Infer stays with the caller. */
void Get_Ancestral_Probs(t_tree *tree, t_node *d, phydbl *probs);
/* ... of all internal nodes in ONE device call: probs [n_otu - 2][n_pattern][ns], row k = a_nodes[n_otu + k] */
void Get_All_Ancestral_Probs(t_tree *tree, phydbl *probs);

/* The pairwise ML distance matrix BioNJ starts from -- ML_Dist, src/lk.c:1783-1906, with the reference's own starting values
   (K80_dist / JC69_Dist by state, formed with the host's libm) -- evaluated on the device (phyhip_calculate_pairwise_ml_distances),
   for a tree made with Make_Tree_For_Lk whose tips and model are loaded.  min_diff_lk_local: mod->s_opt->min_diff_lk_local (1e-3 by
   default).  dist: [n_otu][n_otu], symmetric, diagonal 0, at most DIST_MAX.  One category of rate 1, whatever the model's rate
   classes (ML_Dist forces this).  Fill_Missing_Dist and Bionj stay with the caller. */
void ML_Dist(t_tree *tree, phydbl min_diff_lk_local, phydbl *dist);

/* SH-like branch supports on the device (phyhip_calculate_sh_support; src/alrt.c).  aLRT() runs NNI_Neigh_BL per internal edge,
   which evaluates the three NNI configurations with Lk(b) and keeps c_lnL_sorted of each (src/alrt.c:453,555,682):
   Set_Log_Lks_aLRT(tree, k), k = 0..2, is that assignment -- log_lks_aLRT[k][site] = c_lnL_sorted[site] of the Lk(b) that has just
   run -- as a device-to-device snapshot, no download.  Statistics_To_SH (src/alrt.c:1148-1298) and the deprecated Statistics_to_RELL
   (src/alrt.c:1091-1140) then resample the three vectors: 10 000 replicates of tree->init_len sites under tree->wght, draws seeded by
   tree->sh_seed (Philox4x32-10: not the reference's rand() stream, the same estimate).  tree->sh_seed is passed on UNCHANGED: two
   calls with the same seed draw the same replicates, so a caller that wants every internal edge of a tree resampled independently
   -- as the reference's running rand() stream does -- sets tree->sh_seed per edge (its run seed plus b->num, say) before the call.
   Mixture trees are not served. */
void   Set_Log_Lks_aLRT(t_tree *tree, int k);
phydbl Statistics_To_SH(t_tree *tree);
phydbl Statistics_to_RELL(t_tree *tree);

/* ---- parsimony: src/pars.h on the device (phyhip_set_parsimony ...) ---------------------------------------------------------------
   For a tree made with Make_Tree_For_Lk whose tips are loaded: the parsimony buffers are the partials buffers' indices (Prune_Subtree /
   Graft_Subtree swap ui_*, pars_* and p_pars_* together with p_lk_*, src/utilities.c:6269-6278), tips are read from the tip data
   the instance holds.  Names and semantics are the reference's:
     Make_Tree_For_Pars(tree)            src/make.c      tree->site_pars, Get_Step_Mat, parsimony enabled on the instance in the mode
                                                         tree->general_pars says (call it again after changing general_pars)
     Pars(b,tree)                        src/pars.c:20   b == NULL: Post_Order_Pars from a_nodes[0] (+ Pre_Order_Pars with both_sides), then
                                                         a_nodes[0]->b[0] is scored, all in ONE device call; fills tree->site_pars, tree->c_pars
     Update_Partial_Pars(tree,b,n)       src/pars.c:239  one operation queued (children by neighbour position, as Update_Partial_Lk);
                                                         returns at once for a tip, after the alias gate
     Post_Order_Pars / Pre_Order_Pars    src/pars.c:56/77
     Pars_At_Given_Edge(b,tree)          src/pars.c:468
     Update_Pars_At_Given_Edge(b,tree)   src/pars.c:488
     Get_Step_Mat(tree)                  src/pars.c:498  nucleotides (transition 1, transversion 2, ACGT order) and the 0/1 matrix only; a
                                                         step_mat the caller has set is left alone
   c_pars: weights that are whole numbers give the exact sum (as the reference's int holds it); any other weight makes the device
   refuse the sum, and Pars runs the reference's truncating loop c_pars += site_pars * wght itself over the downloaded site_pars.
   Not built: rooted trees (tree->e_root) and mixture trees exit with "not built". */
void Make_Tree_For_Pars(t_tree *tree);
void Free_Tree_Pars(t_tree *tree);
int  Pars(t_edge *b, t_tree *tree);
void Update_Partial_Pars(t_tree *tree, t_edge *b_fcus, t_node *n);
void Post_Order_Pars(t_node *a, t_node *d, t_tree *tree);
void Pre_Order_Pars(t_node *a, t_node *d, t_tree *tree);
int  Pars_At_Given_Edge(t_edge *b, t_tree *tree);
int  Update_Pars_At_Given_Edge(t_edge *b_fcus, t_tree *tree);
void Get_Step_Mat(t_tree *tree);
/* download hooks: the side of b at node d -- ui / pars [n_pattern] (Fitch) or p_pars [n_pattern][ns] (step matrix); NULL: not wanted */
void Get_Partial_Pars(t_tree *tree, t_edge *b, t_node *d, int *ui, int *pars, int *p_pars);
void Get_Site_Pars(t_tree *tree, int *site_pars);
/* The parsimony regraft scan of one pruned subtree in ONE device call (phyhip_calculate_regraft_parsimony): what Test_One_Spr_Target
   (src/spr.c:639-651) computes target by target under spr_pars == YES -- Update_Partial_Pars(b_arrow, n_link), Pars(b_arrow) -- for n
   target edges at once.  The subtree is the vector of b_sub on d_sub's side (d_sub a tip: its tip vector); candidate i joins the two
   side vectors of b_target[i] (the right one is the tip where rght->tax); buffer indices are resolved as Lk_Regraft_Scan resolves
   them.  pars[i]: what Pars(b_arrow) would leave in tree->c_pars for candidate i.  keep (-1: none): the candidate whose joined
   vector and per-pattern scores stay for Get_Regraft_Partial_Pars / Get_Regraft_Site_Pars (shapes as Get_Partial_Pars /
   Get_Site_Pars).  Updates queued with Update_Partial_Pars before the call (the path updates of Test_One_Spr_Target_Recur,
   src/spr.c:545) are seen.  tree->c_pars, tree->site_pars and every plane are left alone.  The call is always the scan: batching
   is the caller's choice.  A sum above INT_MAX (the reference's c_pars is an int), a weight that is not a whole number or any
   refusal of the device call (include/phyhip.h) runs the exit handler; the caller then takes the targets one by one.
   This layer has no Prune_Subtree / Graft_Subtree: on an INTACT tree the vectors are whatever the tree holds -- the side vectors of a
   target edge still contain the subtree, so the numbers are those of the call sequence, not of a legal SPR move; a caller that has
   pruned (tests/test_gpu_pars_regraft.py drives the device call over the pruned topology) gets the search's candidates. */
void Pars_Regraft_Scan(t_tree *tree, t_edge *b_sub, t_node *d_sub, int n, t_edge *const *b_target, int keep, int *pars);
void Get_Regraft_Partial_Pars(t_tree *tree, int *ui, int *pars, int *p_pars);
void Get_Regraft_Site_Pars(t_tree *tree, int *site_pars);

void Set_Exit_Handler(void (*handler)(const char *msg));

#ifdef __cplusplus
}
#endif
#endif
