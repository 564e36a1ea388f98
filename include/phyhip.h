/*
 * phyhip.h -- C ABI of the MI355X-native Felsenstein-pruning likelihood engine (libphyhip.so).
 *
 * This is the drop-in boundary of SURVEY.md section 8b: PhyML's only accelerator seam is the
 * `#ifdef BEAGLE` hook (src/lk.c:1300-1302, :585-587, :2327-2367; src/beagle_utils.c), whose foreign
 * calls are the BEAGLE C API.  Every entry point below names the call of that seam it replaces
 * (reference file:line) and keeps its argument order and meaning, so the glue a PhyML maintainer adds
 * is a rename.  The numerical semantics, however, are those of PhyML's own AVX path
 * (src/avx.c, src/lk.c) -- in particular PhyML's power-of-two rescaling rule (threshold 2^-256, factor
 * 2^256, one int per pattern and partial buffer: src/avx.c:460-513) instead of BEAGLE's scale
 * buffers, the 1e-100 floor / row renormalisation of transition matrices (src/models.c:293-298) and
 * the [l_min,l_max] clamp of rate-scaled branch lengths (src/lk.c:2296-2300) -- because the parity
 * target is the AVX path, not BEAGLE (the manual quotes 1e-4 disagreement for the latter).
 *
 * Plain C: ints, doubles, pointers and sizes only.  One host thread drives one instance (the
 * reference is single-threaded and non re-entrant).  All functions return
 * PHYHIP_SUCCESS (0) or a negative PHYHIP_ERROR_* code; phyhip_get_last_error() gives the text.
 * The glue prints it and calls Exit(), as src/beagle_utils.c:246-249 does.
 *
 * Data layouts (identical to the reference's host buffers, so uploads/downloads are memcpys):
 *   partials buffer   [pattern][category][state]  double     (t_edge::p_lk_left/p_lk_rght)
 *   tip partials      [pattern][state]            double 0/1 (t_edge::p_lk_tip_r)
 *   scale factors     [pattern]                   int        (t_edge::sum_scale_left/rght)
 *   transition matrix [category][from][to]        double     (t_edge::Pij_rr)
 *
 * Buffer index space (as in src/beagle_utils.c:108-113, lk.c:2221-2230): partial-buffer indices
 * 0..tipCount-1 are the tips, tipCount..partialsBufferCount-1 are internal edge sides.
 *
 * Execution model: phyhip_update_partials() only *queues* operations; the queue is flushed as ONE
 * kernel launch (the whole post-order traversal for every pattern tile) by the first call that needs
 * results: phyhip_calculate_edge_log_likelihoods*, phyhip_get_*, phyhip_update_eigen_lr,
 * phyhip_synchronize.  Callers need not know this; results are as if every call were synchronous.
 */
#ifndef PHYHIP_H
#define PHYHIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PHYHIP_SUCCESS                         0
#define PHYHIP_ERROR_GENERAL                  (-1)
#define PHYHIP_ERROR_OUT_OF_MEMORY            (-2)
#define PHYHIP_ERROR_UNIDENTIFIED_EXCEPTION   (-3)
#define PHYHIP_ERROR_UNINITIALIZED_INSTANCE   (-4)
#define PHYHIP_ERROR_OUT_OF_RANGE             (-5)
#define PHYHIP_ERROR_NO_RESOURCE              (-6)   /* no gfx950 device visible */
#define PHYHIP_ERROR_NO_IMPLEMENTATION        (-7)
#define PHYHIP_ERROR_FLOATING_POINT           (-8)

#define PHYHIP_OP_NONE (-1)   /* BEAGLE_OP_NONE */

/* requirementFlags bit of phyhip_create_instance: build the sharded (multi-device) form even for a resource list of
   ONE device -- same code path, communicator of one rank (used by the single-GPU tests of that path). */
#define PHYHIP_FLAG_SHARDED (1L << 40)
#define PHYHIP_UNIQUE_ID_BYTES 128 /* sizeof(ncclUniqueId) */
/* requirementFlags bit: the categoryCount "categories" of the instance are the CLASSES of a mixture of class models
   (src/mixt.c; e.g. the four classes of LG4X): class c has its own eigen system and frequencies (eigenIndex / 
   stateFrequenciesIndex = c), its category rate is the class rate, every partials buffer carries one scale vector per
   class, and evaluations go through phyhip_calculate_class_mixture_*.  20 states x up to 4 classes, or 4 states x 1, 2 or 4
   classes; with a resource list the instance is sharded like any other (one all-reduce per mixture evaluation). */
#define PHYHIP_FLAG_CLASS_AXIS (1L << 41)
/* requirementFlags bit: the arithmetic of the reference's GENERIC partial-likelihood loop (Update_Partial_Lk_Generic,
   src/lk.c:1332-1587) as `phyml --cov` runs it on 4- or 20-state data (mod->use_m4mod, src/cl.c:753-757, src/lk.c:1303-1324):
   no all-ones shortcut -- a fully ambiguous subtree yields the rounded row sums of the transition matrices instead of exactly
   1.0 -- everything else as the default path (the same fused multiply-add chains; pinned by tests/golden/nucleic_cov_generic.phyg).
   Served by the plain, non-pipelined kernel: the door is there for parity, the reference itself runs it at half speed. */
#define PHYHIP_FLAG_GENERIC_LOOP (1L << 42)

/* BeagleOperation (src/beagle_utils.c:243).  The two scale-index fields are accepted and ignored:
   scale vectors are implicit, one per partials buffer, as in PhyML. */
typedef struct
{
  int destinationPartials;
  int destinationScaleWrite;
  int destinationScaleRead;
  int child1Partials;
  int child1TransitionMatrix;
  int child2Partials;
  int child2TransitionMatrix;
} phyhip_operation;

/* BeagleInstanceDetails (src/beagle_utils.c:84-95) */
typedef struct
{
  int  resourceNumber;     /* HIP device ordinal */
  char resourceName[64];   /* e.g. "AMD Instinct MI355X" */
  char implName[64];       /* "phyhip-gfx950" */
  long flags;
  int  computeUnits;
  long long globalMemBytes;
} phyhip_instance_details;

/* ---- instance lifetime ------------------------------------------------------------------ */

/* replaces beagleCreateInstance, src/beagle_utils.c:119-133.
   compactBufferCount, scaleBufferCount, preferenceFlags are accepted for signature compatibility;
   resourceList[0] (if given) is the HIP device ordinal, else env PHYHIP_DEVICE, else 0.
   MULTI-GPU: a resource list of G > 1 devices creates ONE sharded instance -- patterns are split into G
   contiguous ranges [g*P/G, (g+1)*P/G), one per listed device (a device may be listed more than once), everything
   per-pattern (tips, weights, invariant sites, partials, scale vectors, per-site outputs) is sliced / concatenated by
   the entry points below, the model and the transition matrices are replicated, and every scalar-returning evaluation
   (phyhip_calculate_edge_log_likelihoods, phyhip_calculate_eigen_lnl[_dlnl]) ends in ONE RCCL all-reduce over the
   communicators of ncclCommInitAll: {warning flag, lnL} for Lk (the sum of src/lk.c:856), {warning, lnL, dlnL} for dLk
   (src/lk.c:744-745).  The caller sees the same API and the same numbers; mixture evaluations (below) accept sharded class instances too.
   Returns the instance id (>= 0) or a negative error. */
int phyhip_create_instance(int tipCount, int partialsBufferCount, int compactBufferCount, int stateCount,
                           int patternCount, int eigenBufferCount, int matrixBufferCount, int categoryCount,
                           int scaleBufferCount, const int *resourceList, int resourceCount,
                           long preferenceFlags, long requirementFlags, phyhip_instance_details *returnInfo);

/* replaces beagleFinalizeInstance, src/beagle_utils.c:266 */
int phyhip_finalize_instance(int instance);

const char *phyhip_get_last_error(void);

/* ---- inputs ---------------------------------------------------------------------------------- */

/* replaces beagleSetTipPartials, src/beagle_utils.c:153.  inPartials is [pattern][state] with 0/1
   entries (src/lk.c:26-161); it is stored on the device as one byte per pattern (an index into a
   table of allowed-state masks).  Entries other than 0 and 1 are rejected (PHYHIP_ERROR_OUT_OF_RANGE). */
int phyhip_set_tip_partials(int instance, int tipIndex, const double *inPartials);

/* replaces beagleSetTipStates (BEAGLE compact form): state in [0,stateCount) or >= stateCount for a
   fully ambiguous character. */
int phyhip_set_tip_states(int instance, int tipIndex, const int *inStates);
/* One pattern of one tip rewritten in place: inPartials[stateCount] of 0.0 / 1.0, as a row of phyhip_set_tip_partials.
   Init_Partial_Lk_Tips_Double_One_Character (src/lk.c:2092), the tip rewrite of the leave-one-out cross-validation loops
   (src/mixt.c:4225-4258, src/cv.c:51-118).  Takes effect in stream order, without a host synchronisation for the single states and
   for "every state" (the hidden character of the leave-one-out loop: its table entry exists from instance creation); on
   20-state instances the FIRST use of any other state set adds an entry to the device's table of state sets, which costs one
   stream synchronisation.  A row with no state allowed is rejected (PHYHIP_ERROR_OUT_OF_RANGE).  Partial vectors that depend
   on the tip are the caller's to update, as in the reference. */
int phyhip_set_tip_partials_at_pattern(int instance, int tipIndex, int pattern, const double *inPartials);

/* replaces beagleSetPartials: upload an internal partials buffer ([pattern][category][state]). */
int phyhip_set_partials(int instance, int bufferIndex, const double *inPartials);

/* replaces beagleSetPatternWeights, src/beagle_utils.c:165 (re-callable: bootstrap re-weights,
   src/utilities.c:3945-3955).  Patterns with weight <= DBL_MIN are skipped in every sum. */
int phyhip_set_pattern_weights(int instance, const double *inPatternWeights);

/* replaces beagleSetCategoryRates / beagleSetCategoryWeights, src/beagle_utils.c:281-305 */
int phyhip_set_category_rates(int instance, const double *inCategoryRates);
int phyhip_set_category_weights(int instance, int categoryWeightsIndex, const double *inCategoryWeights);

/* replaces beagleSetStateFrequencies, src/beagle_utils.c:322-325 */
int phyhip_set_state_frequencies(int instance, int stateFrequenciesIndex, const double *inStateFrequencies);

/* replaces beagleSetEigenDecomposition, src/beagle_utils.c:383-386.  inEigenVectors = r_e_vect,
   inInverseEigenVectors = l_e_vect (row-major [state][state]); inEigenValues are the RAW eigenvalues
   of Q (mod->eigen->e_val, src/models.c:275 -- the log() in beagle_utils.c:376 is stale). */
int phyhip_set_eigen_decomposition(int instance, int eigenIndex, const double *inEigenVectors,
                                   const double *inInverseEigenVectors, const double *inEigenValues);

/* PhyML-specific knobs the BEAGLE API has no slot for.
   l_min,l_max: mod->l_min/l_max (src/init.c:711-714); br_len_mult: mod->br_len_mult->v;
   apply_lk_scaling: tree->apply_lk_scaling (src/utilities.h:993). */
int phyhip_set_phyml_options(int instance, double l_min, double l_max, double br_len_mult, int apply_lk_scaling);

/* +I model: mod->ras->invar, mod->ras->pinvar->v, data->invar[pattern] (src/lk.c:820-842,1226-1273).
   invar may be NULL when invar_model == 0. */
int phyhip_set_invariant_sites(int instance, int invar_model, double pinvar, const short *invar);

/* ---- transition matrices --------------------------------------------------------------------- */

/* replaces beagleUpdateTransitionMatrices, src/lk.c:2344.  For each i < count builds, on the device,
   all categories of matrix probabilityIndices[i] for edge length edgeLengths[i] (= b->l->v; the MAX(0,.)
   x rate x br_len_mult product and the clamp of src/lk.c:2296-2300 are applied here), with the
   floor / renormalise post-processing of src/models.c:293-298.  Derivative indices must be NULL. */
int phyhip_update_transition_matrices(int instance, int eigenIndex, const int *probabilityIndices,
                                      const int *firstDerivativeIndices, const int *secondDerivativeIndices,
                                      const double *edgeLengths, int count);

/* replaces beagleSetTransitionMatrix, src/lk.c:2360: upload b->Pij_rr ([category][from][to]) as computed
   by the host's own PMat() -- bit-exact by construction.  (phyhip_update_transition_matrices above builds the
   same doubles on the device: its exp() is the reference's libm's, phyml_amd/csrc/phyhip_exp.hpp.) */
int phyhip_set_transition_matrix(int instance, int matrixIndex, const double *inMatrix, double paddedValue);

/* replaces beagleGetTransitionMatrix, src/lk.c:2351 */
int phyhip_get_transition_matrix(int instance, int matrixIndex, double *outMatrix);

/* ---- the hot path ---------------------------------------------------------------------------- */

/* replaces beagleUpdatePartials, src/beagle_utils.c:245 (i.e. the body of Update_Partial_Lk,
   src/lk.c:1300-1302 -> src/avx.c:301-522).  Operations are executed in order; an operation may read
   the destination of an earlier one, but not its own (PHYHIP_ERROR_OUT_OF_RANGE: Update_Partial_Lk never
   updates in place).  cumulativeScaleIndex is ignored. */
int phyhip_update_partials(int instance, const phyhip_operation *operations, int operationCount,
                           int cumulativeScaleIndex);

/* replaces beagleCalculateEdgeLogLikelihoods, src/beagle_utils.c:344 (i.e. the site loop of Lk(),
   src/lk.c:590-645 + Lk_Core :767-861).  count must be 1.  parentBufferIndices[0] is b->p_lk_left,
   childBufferIndices[0] the right side (tip index if b->rght->tax), probabilityIndices[0] b->Pij_rr.
   Derivative outputs must be NULL (PhyML differentiates in the eigen basis: phyhip_calculate_eigen_*). */
int phyhip_calculate_edge_log_likelihoods(int instance, const int *parentBufferIndices,
                                          const int *childBufferIndices, const int *probabilityIndices,
                                          const int *firstDerivativeIndices, const int *secondDerivativeIndices,
                                          const int *categoryWeightsIndices, const int *stateFrequenciesIndices,
                                          const int *cumulativeScaleIndices, int count,
                                          double *outSumLogLikelihood, double *outSumFirstDerivative,
                                          double *outSumSecondDerivative);

/* Same evaluation, but the sum stays in device memory (deviceOut[0] = lnL) and the call does not synchronise
   (callers that run their own collective; the library's own multi-GPU forms are described at phyhip_create_instance
   and phyhip_comm_init_rank). */
int phyhip_calculate_edge_log_likelihoods_device(int instance, int parentBufferIndex, int childBufferIndex,
                                                 int probabilityIndex, double *deviceOut);

/* replaces beagleGetSiteLogLikelihoods, src/beagle_utils.c:355 (log-likelihood per pattern,
   tree->c_lnL_sorted) */
int phyhip_get_site_log_likelihoods(int instance, double *outLogLikelihoods);

/* The other per-pattern outputs of Lk_Core that host readers use (src/lk.c:855-857, 2791, 2801);
   any pointer may be NULL.  (Class-axis instances: fact_sum_scale holds categoryCount x patternCount ints, [class][pattern].) */
int phyhip_get_site_outputs(int instance, double *c_lnL_sorted, double *cur_site_lk,
                            double *unscaled_site_lk_cat, int *fact_sum_scale);

/* The per-pattern outputs of Lk_Core at one edge as the REFERENCE's doubles, bit for bit -- what host readers that compare or
   rank them need (aLRT / SH-like supports, --print_site_lnl, cv.c, ancestral reconstruction).  phyhip_get_site_outputs returns
   what the last evaluation of the hot path left: equal to the reference to 1e-10 / 1e-12 only (the evaluation kernels take the
   general product for every pattern and the device library's log).  This call evaluates the edge again in a kernel of its own,
   operation by operation as Lk_Core does (src/lk.c:767-861, src/avx.c:110-215, Pull_Scaling_Factors): the tip branch
   pi[s] * norm(P[s][.] o left) where the child is a tip with exactly one allowed state, the general product elsewhere, the +I
   mixing with Invariant_Lk's overflow branch, the SMALL floor (-> *outNumericalWarning = 1), glibc's log and exp.
     parent = left side, child = right side; either may be a tip index.  Precondition as in the reference: the partials on both
   sides are current (queued operations are executed first, virtual buffers stored).  Any output pointer may be NULL.
     c_lnL_sorted, cur_site_lk [pattern]; unscaled_site_lk_cat [pattern][category]; fact_sum_scale [pattern].  Entries of
   patterns whose weight is not above SMALL are written as 0 (the reference leaves them stale).
     *outSumLogLikelihood: the sum over the patterns in ascending order of the rounded products weight x c_lnL_sorted (src/lk.c:856),
   formed on the host -- for a sharded instance over all its patterns, so sharding does not change it.
     Nothing else changes: the outputs of the last evaluation (phyhip_get_site_outputs, phyhip_get_site_log_likelihoods), the
   numerical warning, every partial, scale vector and matrix stay what they were.
     One-process-per-GPU form (phyhip_comm_init_rank): the call is LOCAL to the rank -- its own patterns, its own sum, no collective.
     Instances created with PHYHIP_FLAG_CLASS_AXIS or PHYHIP_FLAG_GENERIC_LOOP: PHYHIP_ERROR_NO_IMPLEMENTATION.  1 .. 64 categories. */
int phyhip_calculate_edge_site_outputs_exact(int instance, int parentBufferIndex, int childBufferIndex,
                                             int probabilityIndex,
                                             double *c_lnL_sorted, double *cur_site_lk,
                                             double *unscaled_site_lk_cat, int *fact_sum_scale,
                                             double *outSumLogLikelihood, int *outNumericalWarning);

/* The marginal posterior of every state at internal nodes -- the site loop of Ancestral_Sequences_One_Node (src/ancestral.c:609-901,
   what `phyml --ancestral` prints) -- evaluated on the device for a list of nodes in one launch, so that only the answer crosses
   the link instead of every partial and scale vector of the tree (phyhip_get_partials / phyhip_get_scale_factors).
     Node k has neighbours v_0..v_2 over edges b_0..b_2.  sideBufferIndices[3k+j]: the partials buffer of b_j on v_j's side
   (v_j == b_j->left ? p_lk_left : p_lk_rght), or v_j's tip index where v_j is a tip; probabilityIndices[3k+j]: the matrix of b_j
   ([category][i][j], as everywhere).  Per pattern p and state i:
       x_j(c,i) = sum_s side_j[p][c][s] * Pij_j[c][i][s]      (a tip: its allowed-state 0/1 vector in every category)
       q[i]     = sum_c x_0 x_1 x_2 pi[i] gamma_r_proba[c];   ss = the scale exponents of the non-tip sides at p, added
       +I:        q[i] = q[i] (1 - pinvar) + Invariant_Lk(ss, p) pinvar pi[i]; where Invariant_Lk overflowed (-> *outNumericalWarning
                  = 1) q[i] = Invariant_Lk(0, p) pinvar pi[i]                                   (src/ancestral.c:843-865)
       outPosteriors[k][p][i] = exp(log(q[i]) - LOG2 ss - c_lnL_sorted[p])                     (src/ancestral.c:868-870)
   inSiteLogLikelihoods: c_lnL_sorted [pattern], or NULL for what the instance's last edge evaluation left on the device
   (phyhip_get_site_log_likelihoods) -- the reference runs this after Set_Both_Sides(YES); Lk(NULL) (src/main.c:281-288).
     Precondition as in the reference: the partials on all three sides of every node are current (queued operations are executed
   first, virtual buffers stored).  Rows of patterns whose weight is not above SMALL are written as 0 (the reference reads stale
   vectors there).  *outNumericalWarning (may be NULL) is 0 unless Invariant_Lk overflowed at some pattern.  nodeCount == 0 succeeds.
     NO bit parity with the reference's binary is claimed for this call: the reference's products run in plain C order under -O3
   contraction, which nothing pins; this kernel's order of additions is its own.  It is held to the formula above at 1e-10
   relative per entry; log and exp are the reference's libm's.  MPEE_Infer is a host function of the result and stays with the caller.
     Nothing else changes: partials, scale vectors, matrices, the outputs of the last evaluation, the numerical warning and what
   the next evaluation returns stay what they were.  The result's device work space (nodeCount x patternCount x stateCount
   doubles) is allocated or grown on use and kept; if it cannot be had: PHYHIP_ERROR_OUT_OF_MEMORY -- ask for fewer nodes per call.
     Sharded instance: each shard computes its pattern range and the rows land at their global pattern positions; sharding changes
   no bit of the result.  One-process-per-GPU form (phyhip_comm_init_rank): LOCAL to the rank, no collective.
     Bad side or matrix indices: PHYHIP_ERROR_OUT_OF_RANGE.  Instances created with PHYHIP_FLAG_CLASS_AXIS or
   PHYHIP_FLAG_GENERIC_LOOP: PHYHIP_ERROR_NO_IMPLEMENTATION.  1 .. 64 categories, 4 or 20 states. */
int phyhip_calculate_node_state_posteriors(int instance, int nodeCount,
                                           const int *sideBufferIndices, const int *probabilityIndices,
                                           const double *inSiteLogLikelihoods, double *outPosteriors,
                                           int *outNumericalWarning);

/* The pairwise maximum-likelihood distance matrix that BioNJ turns into the starting tree: ML_Dist (src/lk.c:1783-1906) with
   Lk_Dist (src/lk.c:2416-2473) under Opt_Dist_F / Dist_F_Brent (src/optimiz.c:1848-1972), started from K80_dist / JC69_Dist
   (src/utilities.c:2407-2587) -- what Dist_And_BioNJ runs on every run without -u, Add_BioNJ_Branch_Lengths, and every bootstrap
   replicate (src/utilities.c:4000, src/mpi_boot.c:177) -- evaluated on the device from the tips the instance holds.  For every pair
   of tips j < k, with ONE rate category of rate 1 and weight 1 (ML_Dist forces this: the instance's category rates and weights are
   ignored):
       F[s0][s1] = sum of the weights of the patterns where BOTH tips have exactly one allowed state (a one-hot tip vector; on this
                   ABI B / Z are the single states N / Q); len = sum F; F /= len where len > 0
       init      = 4 states, K80_dist(data, 1e6): P = transitions / len, Q = transversions / len (both .5 where len == 0);
                     -1 where 1-2P-Q <= 0 or 1-2Q <= 0, else (g/2)(pow(1-2P-Q,-1/g) + 0.5 pow(1-2Q,-1/g) - 1.5), g = 1e6, at most DIST_MAX = 2
                   else JC69_Dist: P = mismatches / len (1 where len == 0); -1 where 1 - (S/(S-1))P < 0, else
                     -((S-1)/S) log(1 - (S/(S-1))P), at most DIST_MAX
                   then 0.1 where init > DIST_MAX - SMALL or init < 0
       d         = init where sum F < .001 (no common unambiguous site); else Dist_F_Brent(l_min, max(init, l_min), l_max, 1e-10, 1000)
                   on -Lk_Dist(F, |u|), which stops when |curr_lnL - old_lnL| < minDiffLk && curr_lnL > init_lnL - minDiffLk
                   (minDiffLk: mod->s_opt->min_diff_lk_local, 1e-3 by default, src/init.c:770);
                   Lk_Dist(F, d) = sum_{i<j} (F[i][j] + F[j][i]) log(pi[i] P[i][j]) + sum_i F[i][i] log(pi[i] P[i][i]), P =
                   PMat_Empirical(d clamped to [l_min, l_max]) of eigen system eigenIndex, SMALL_PIJ floor and row
                   renormalisation included, pi = frequencies stateFrequenciesIndex
       outDistances[j][k] = outDistances[k][j] = min(d, DIST_MAX); the diagonal is 0
   l_min / l_max are those of phyhip_set_phyml_options.  mod->log_l is not served.  Mixtures: the binding picks the class by its
   eigen index (the reference uses the first class).  Fill_Missing_Dist and BioNJ are O(n^2) / O(n^3) host work without a pattern
   axis and stay with the caller.
     The STARTING VALUES are formed on the host side of this library with libm's pow / log, from sums the device reduced: the
   optimiser stops long before convergence, so its answer follows its starting value one for one, and K80's formula multiplies the
   last bit of pow by 5e5.  Counting by state departs from the reference's counting by character in two places: K80_dist skips a
   'U' (here it is the state T), and JC69_Dist counts B against N and Z against Q as mismatches (here they are the same state).
   A binding that needs those passes its own matrix as inInitialDistances ([tip][tip], K80_dist's / JC69_Dist's output, -1 where
   the closed form is invalid; only j < k is read); the round trip of the sums is then skipped.
     Optional outputs (each may be NULL): outInitialDistances [tip][tip], what the closed form gave BEFORE the 0.1 rule;
   outCounts [pair][state][state], the normalised F, pairs in the order (0,1), (0,2), .., (1,2), ..; outLogLikelihoods [pair],
   Lk_Dist at the returned distance before the DIST_MAX cap (0 where sum F < .001); outIterations [pair], the iteration of
   Dist_F_Brent that returned (0 where sum F < .001).
     Numbers: the raw counts are exact for integer weights and the same bits from run to run for any weights (one fixed order
   of additions per entry, no atomics); patterns whose weight is not above SMALL contribute nothing.  Matrices, exp and log are
   the reference's doubles; Lk_Dist's sum runs in the reference's order, so the distances differ from the reference binary's by
   its compiler's contraction only (1e-9 relative on the reference's own examples).
     Nothing else changes: partials, scale vectors, matrices, the outputs of the last evaluation and the numerical warning stay
   what they were, and no queued operation is executed.  The device work space (the raw counts of a band of taxa, at most
   phyhip_set_pairwise_work_space bytes, and a few doubles per pair) is allocated or grown on use and kept; if it cannot be
   had: PHYHIP_ERROR_OUT_OF_MEMORY.
     Sharded instance (one process): each shard counts its patterns on its own device, the raw counts are added in shard order
   on the first shard's device, the rest runs there.  Instances of phyhip_comm_init_rank (a rank holds only its own patterns),
   PHYHIP_FLAG_CLASS_AXIS and PHYHIP_FLAG_GENERIC_LOOP instances: PHYHIP_ERROR_NO_IMPLEMENTATION.  Bad eigen / frequency index,
   minDiffLk <= 0: PHYHIP_ERROR_OUT_OF_RANGE.  4 or 20 states. */
int phyhip_calculate_pairwise_ml_distances(int instance, int eigenIndex, int stateFrequenciesIndex,
                                           double minDiffLk,
                                           const double *inInitialDistances,
                                           double *outDistances,
                                           double *outInitialDistances,
                                           double *outCounts,
                                           double *outLogLikelihoods,
                                           int *outIterations);

/* Bound, in bytes, on the raw counts phyhip_calculate_pairwise_ml_distances holds at a time (it walks the taxa in bands of as many
   as fit, at least one; with more than one band and no inInitialDistances the counts are formed twice).  0: the default, 128 MiB.
   No result depends on it. */
int phyhip_set_pairwise_work_space(int instance, long long maxBytes);

/* SH-like branch supports: the resampling of Statistics_To_SH (src/alrt.c:1148-1298, reached by `-b -4` and `-b -2`) -- and of the
   deprecated Statistics_to_RELL (src/alrt.c:1091-1140), which falls out of the same pass -- evaluated on the device.  For every
   internal edge aLRT (src/alrt.c:172-226) runs NNI_Neigh_BL, which stores c_lnL_sorted of the three NNI configurations in
   log_lks_aLRT[0..2] (src/alrt.c:453,555,682); the statistic then draws 10 000 replicates of init_len sites each: 10 000 x init_len
   draws per internal edge on one host thread, against three evaluations that take micro- to milliseconds here.

   phyhip_set_support_site_log_likelihoods fills slot 0..2 with one per-pattern vector [pattern]: from the host pointer, or -- NULL --
   with what the instance's last edge evaluation left on the device (what phyhip_get_site_log_likelihoods would return), device to
   device, with no download: log_lks_aLRT[slot][site] = c_lnL_sorted[site].  A NULL snapshot executes queued operations first, as
   that getter does.  The slots (3 x patternCount doubles) are allocated on first use and kept.  Nothing else moves: partials, scale
   vectors, matrices, the outputs of the last evaluation, the numerical warning and the next evaluation stay what they were. */
int phyhip_set_support_site_log_likelihoods(int instance, int slot, const double *inSiteLogLikelihoods);

/* The statistic from the three slots.  Weights w: the instance's pattern weights (phyhip_set_pattern_weights); siteCount: data->init_len;
   replicateCount: 10 000 in the reference.
       c_k       = sum over the patterns in ascending order of slot_k[p] * w[p] (the rounded product, then the addition;
                   src/alrt.c:1172-1177): one fixed order of additions.  outTotals[k] = c_k.
       delta     = the gap between the largest and the second largest of c_0..c_2, by the six-way ordering of src/alrt.c:1184-1216
                   restated line by line, ties (>=) included
       replicate r: siteCount draws of a pattern with probability w[p] / sum w;  lk_k = sum over the draws of slot_k[drawn pattern]
                   (outReplicateSums[r][k], may be NULL: these UNCENTRED sums);  RELL: lk_0 >= lk_1 && lk_0 >= lk_2 (src/alrt.c:1129);
                   lk_k -= c_k (src/alrt.c:1249-1251);  delta_local by the same ordering of the centred sums (src/alrt.c:1254-1287);
                   accepted (outAccepted[r] = 0 / 1, may be NULL) when delta > delta_local + 0.1 (src/alrt.c:1289)
       *outSH    = accepted replicates / replicateCount;  *outRELL = RELL replicates / replicateCount      (each may be NULL)
   THE ALIAS TABLE is Sample_n_i_With_Proba_pi's (src/stats.c:4493-4560), built operation for operation on the host side of this
   library in plain sequential C, O(patternCount): pi = w / siteCount, their sum, p = pi * patternCount / sum, the descending fill of
   small / large, the pairing loop p[g] = p[g] + p[a] - 1, the leftovers set to 1 (alias 0).  It is built once per weight vector and
   siteCount and kept until phyhip_set_pattern_weights is called; phyhip_get_support_alias_table returns it (prob [pattern], alias
   [pattern], either may be NULL) so that a test can hold it.
     THE DRAWS are not the reference's: its rand() stream is sequential and cannot be the device's (src/stats.c:4566-4572 takes two
   rand() per draw).  They come from Philox4x32-10 (Salmon et al. 2011), counter-based and integer-only, so that an independent
   restatement reproduces every draw bit for bit: key = (seed low word, seed high word), counter = (j, 0, r, 0) for draw pair j of
   replicate r; draw 2j takes the output words (w0, w1), draw 2j+1 takes (w2, w3) -- dropped when siteCount is odd and 2j+1 ==
   siteCount.  column = (w_a * patternCount) >> 32 (unlike (int)(len * r1) this can never index patternCount); the draw keeps the
   column if w_b * 2^-32 < prob[column], else takes alias[column].  A replicate's draws depend on (seed, r, j) only -- not on
   replicateCount, not on the launch geometry.  The support is therefore a Monte-Carlo estimate of the same probability as the
   reference's, not the same number: two runs of the reference with different srand() differ the same way.
     Numbers: one wave per replicate; lane l adds the draws of the pairs l, l + 64, .. in ascending order, the 64 partial sums meet
   in a fixed butterfly (lane distance 32, 16, .., 1).  No floating-point atomics: the same bits from run to run, for any grid size
   and any replicateCount.  Each sum lies within siteCount x 2^-52 x sum |terms| of the exact sum of its draws, each total within
   patternCount x 2^-52 x sum |terms|.  Per draw the kernel gathers one 64-byte row {prob, the column's three values, its alias's
   three values} of a table it rebuilds per call from the slots.
     Nothing else changes: partials, scale vectors, matrices, the outputs of the last evaluation and the numerical warning stay what
   they were, and no queued operation is executed.  The device work space (about 88 bytes per pattern and 32 per replicate) is
   allocated or grown on use and kept; if it cannot be had: PHYHIP_ERROR_OUT_OF_MEMORY.
     Sharded instance (one process): the slots live on the first shard's device -- a NULL snapshot copies each shard's pattern range
   to its global offset there -- and the rest runs on that device; sharding changes no bit of the result.  Instances of
   phyhip_comm_init_rank (a rank holds only its own patterns), PHYHIP_FLAG_CLASS_AXIS and PHYHIP_FLAG_GENERIC_LOOP instances:
   PHYHIP_ERROR_NO_IMPLEMENTATION; mixture trees (the next_mixt loop of the reference) are not served.  slot outside 0..2,
   siteCount <= 0, replicateCount <= 0, a slot never set, a negative weight, all weights zero (the reference exits at the last two):
   PHYHIP_ERROR_OUT_OF_RANGE.  4 or 20 states are irrelevant here: one kernel. */
int phyhip_calculate_sh_support(int instance, int siteCount, int replicateCount, unsigned long long seed,
                                double *outSH, double *outRELL, double *outTotals,
                                double *outReplicateSums, int *outAccepted);
int phyhip_get_support_alias_table(int instance, int siteCount, double *outProb, int *outAlias);

/* replaces beagleGetPartials, src/beagle_utils.c:252 (download hook for ancestral.c, cv.c, m4.c ...) */
int phyhip_get_partials(int instance, int bufferIndex, int scaleIndex, double *outPartials);

/* sum_scale_left/rght of a partials buffer ([pattern] ints) */
int phyhip_get_scale_factors(int instance, int bufferIndex, int *outScaleFactors);
int phyhip_set_scale_factors(int instance, int bufferIndex, const int *inScaleFactors);

/* tree->numerical_warning of the last edge evaluation (src/lk.c:847-851) */
int phyhip_get_numerical_warning(int instance, int *outWarning);

/* ---- mixtures of class models ---------------------------------------------- */

/* MIXT_Lk(b, mixt_tree), src/mixt.c:730-1160, for one partition element without +I: every class tree of the mixture
   (n_catg = 1, its own rate matrix / frequencies; src/mixt.c:2603-2640) is one instance whose single category rate is
   the class rate (mixt_tree->mod->ras->gamma_rr[parent_class_number], src/lk.c:2298).  Flushes the queued operations
   of every class instance, evaluates the given edge in each (the Lk_Core calls of src/mixt.c:997-1010) and combines
   the classes per pattern: 2^-sum rescaling, proba * r_mat_weight / rMatWeightSum * e_frq_weight / eFrqWeightSum /
   sumProbas (src/mixt.c:1048-1053), DBL_MIN floor, log, pattern weights of the FIRST instance.  All instances must sit
   on the same device with the same pattern count and one category; up to 64 classes (profile mixtures of the C10-C60 kind:
   one class tree per profile), PHYHIP_ERROR_OUT_OF_RANGE beyond.  The per-pattern log-likelihoods
   (mixt_tree->c_lnL_sorted) are left in the first instance (phyhip_get_site_log_likelihoods).
   GROUPS OF CLASSES: an entry of `instances` may also be an instance created with PHYHIP_FLAG_CLASS_AXIS (below): it stands for
   its C classes, in category order, evaluated by ONE traversal launch; parent / child / matrix indices stay per ENTRY, the
   per-class tables (classProba, rMatWeight, eFrqWeight) run over all classes in list order (entry 0's classes, then entry
   1's, ...; 64 in total).  A mixture of K classes is then ceil(K / 4) traversal launches per evaluation instead of K -- e.g.
   4 + 4 + 2 for ten classes, 4 + 1 for five; with three nucleotide classes 2 + 1 (the nucleotide class axis holds 1, 2 or 4).
   phyhip_calculate_mixture_eigen_lnl_dlnl takes the same lists. */
int phyhip_calculate_mixture_log_likelihood(const int *instances, int count, const int *parentBufferIndices,
                                            const int *childBufferIndices, const int *probabilityIndices,
                                            const double *classProba, const double *rMatWeight, const double *eFrqWeight,
                                            double rMatWeightSum, double eFrqWeightSum, double sumProbas,
                                            double *outSumLogLikelihood);

/* MIXT_dLk(&l, b, mixt_tree), src/mixt.c:2962-3340 (same restrictions): lnL and dlnL/dl of the mixture at length *l of
   the edge whose eigen-basis products every class instance holds (phyhip_update_eigen_lr on each class first, as
   MIXT_Update_Eigen_Lr does).  *l is clamped with the FIRST instance's [l_min,l_max] like src/lk.c:672-673; per class
   the length is scaled by its category rate and br_len_mult and clamped again (src/mixt.c:3056-3083).
   left/rightBufferIndices: the two sides of the class edges (their scale exponents enter the 2^-sum rescaling). */
int phyhip_calculate_mixture_eigen_lnl_dlnl(const int *instances, int count, const int *leftBufferIndices,
                                            const int *rightBufferIndices, double *l, const double *classProba,
                                            const double *rMatWeight, const double *eFrqWeight, double rMatWeightSum,
                                            double eFrqWeightSum, double sumProbas, double *outLnL, double *outDLnL);

/* +I mixtures (src/mixt.c:1079-1112, 3212-3275): the invariant class of the mixture is not a class tree of the device (PhyML
   skips it in every per-class loop); its share -- pi_inv[invar[pattern]] x pinvar mixed into the site likelihood, the
   derivative scaled by (1 - pinvar) -- enters the combination.  Set on the FIRST instance of the class list (or on the
   class-axis instance); invar_model == 0 switches it off.  The class instances themselves keep invar_model = 0. */
int phyhip_set_mixture_invariant_sites(int instance, int invar_model, double pinvar, const short *invar,
                                       const double *piInvariantClass);

/* The same two evaluations on ONE instance created with PHYHIP_FLAG_CLASS_AXIS (class c = category c): the queued
   partial updates of ALL classes and their edge evaluations are one traversal launch (one per class instance above),
   followed by the combination.  The class trees of PhyML's mixture share their topology and their call sequence
   (MIXT_Update_Partial_Lk / MIXT_Update_PMat_At_Given_Edge loop over them, src/mixt.c:1191-1250), so the glue queues an
   operation once -- when the first class tree reports it.  parent / child / matrix indices as for
   phyhip_calculate_edge_log_likelihoods; the per-pattern log-likelihoods are left for phyhip_get_site_log_likelihoods,
   the per-class likelihoods in unscaled_site_lk_cat ([pattern][class]) of phyhip_get_site_outputs. */
int phyhip_calculate_class_mixture_log_likelihood(int instance, int parentBufferIndex, int childBufferIndex, int probabilityIndex,
                                                  const double *classProba, const double *rMatWeight, const double *eFrqWeight,
                                                  double rMatWeightSum, double eFrqWeightSum, double sumProbas,
                                                  double *outSumLogLikelihood);
int phyhip_calculate_class_mixture_eigen_lnl_dlnl(int instance, int leftBufferIndex, int rightBufferIndex, double *l,
                                                  const double *classProba, const double *rMatWeight, const double *eFrqWeight,
                                                  double rMatWeightSum, double eFrqWeightSum, double sumProbas, double *outLnL,
                                                  double *outDLnL);
/* sum_scale vector of class classIndex of a partials buffer (class-axis instances; class 0 = phyhip_get_scale_factors) */
int phyhip_get_class_scale_factors(int instance, int bufferIndex, int classIndex, int *outScaleFactors);

/* ---- eigen-basis branch-length derivative (no BEAGLE counterpart in the seam) ---------------- */

/* Update_Eigen_Lr(b,tree), src/lk.c:1038-1114 / src/avx.c:21-105: fills the instance's dot_prod
   [pattern][category][state] from the two sides of an edge (either side may be a tip).  Flushes the queue first: on
   nucleotide instances up to 2 048 patterns the queued partial update(s) and the products are one launch -- mostly one
   command of the resident evaluator -- and the call returns when the products are in device memory; the products are
   always ordered before whatever the instance is asked next. */
int phyhip_update_eigen_lr(int instance, int leftBufferIndex, int rightBufferIndex);

/* dLk(&l,b,tree), src/lk.c:655-753: clamps *l to [l_min,l_max], returns lnL and dlnL/dl from dot_prod
   and the fact_sum_scale left by the preceding edge evaluation. */
int phyhip_calculate_eigen_lnl_dlnl(int instance, double *l, double *outLnL, double *outDLnL);

/* Lk(b,tree) with use_eigen_lr == YES, src/lk.c:592-603,625-629,866-950 */
int phyhip_calculate_eigen_lnl(int instance, double l, double *outLnL);

int phyhip_get_dot_prod(int instance, double *outDotProd);

/* Br_Len_Opt's search on one edge -- Br_Len_Spline, src/optimiz.c:2244-2470 -- in ONE device call: every probe of the branch
   length is a dLk on the products phyhip_update_eigen_lr has left (the precondition of phyhip_calculate_eigen_lnl_dlnl), and the
   reference's control flow runs in the kernel itself (one workgroup, one plain launch; phyml_amd/csrc/phyhip_brlen.hip).
     *l          in: the start length, as the caller holds it (not clamped).  out: best_l, the reference's *l on return
     initLnL     tree->c_lnL on entry: the caller's Lk(b) of the edge (what fv becomes when the first derivative is already
                 negative, and what best_lnL starts from)
     iterMax     mod->s_opt->brent_it_max (1 .. BRENT_IT_MAX = 1000), tol: mod->s_opt->min_diff_lk_local (> 0)
     outLnL      best_lnL; outDLnL: tree->c_dlnL as the search leaves it (the last probe's, or the first one's where the upper
                 walk ends before its first probe); outEvaluations: the dLk evaluations taken
     outStatus   0 the spline step was taken; 1 / 2 returned from the lower / upper bracket walk (:2280-2285, :2308-2313); where the
                 reference stops the program: 3 no acceptable root (:2372-2376), 4 bracket invariant broken (:2423-2425),
                 5 iter == iterMax (:2463), 6 a NaN length (src/lk.c:671), 7 a bracket walk longer than the host-computed bound
                 of ceil(log(l_max / l_min) / log 1.2) + 2 trips (cannot happen in exact arithmetic)
   Flushes the queue as phyhip_calculate_eigen_lnl_dlnl does, then waits for the stream.  Reads dot_prod and the instance's
   constants; the numerical warning becomes that of the search's last evaluation; partials, matrices, site outputs, dot_prod and
   the queue are left alone.  A plain call: the large-grid resident workgroups leave, the next resident-served call re-validates
   the stream.  Any out pointer may be NULL.
     Not built (PHYHIP_ERROR_NO_IMPLEMENTATION, nothing launched; the caller drives phyhip_calculate_eigen_lnl_dlnl itself, as
   the host layer's Br_Len_Opt does): ranks of phyhip_comm_init_rank, one-process sharded instances (each probe needs every shard's
   sums), PHYHIP_FLAG_CLASS_AXIS instances and any instance of more than one eigen system, PHYHIP_FLAG_GENERIC_LOOP instances,
   states other than 4 / 20, more than 8 categories (the expl table of one evaluation holds 8), more than 16 384 patterns.  That
   last bound is what the call is built and tested for, NOT where it is faster: measured against the chain of
   phyhip_calculate_eigen_lnl_dlnl calls it won at one of thirteen shapes (54 taxa x 382 nucleotide patterns with 22 long searches,
   by 5 % of a pass; searches of more than 8 probes on at most 382 patterns are faster by a quarter, shorter ones slower) and lost
   at every other (profiles/brlen_opt.md); the host layer's Br_Len_Opt takes it only where its caller asks.  NaN *l or initLnL:
   PHYHIP_ERROR_FLOATING_POINT.  iterMax outside 1 .. 1000, tol <= 0: PHYHIP_ERROR_OUT_OF_RANGE. */
int phyhip_optimise_edge_length(int instance, double *l, double initLnL, int iterMax, double tol,
                                double *outLnL, double *outDLnL, int *outEvaluations, int *outStatus);
/* while phyhip_profile(instance, 1): milliseconds of the search kernel (HIP events on the instance's stream), the calls and the
   evaluations they took since the previous read; reading resets all three */
int phyhip_profile_read_edge_length(int instance, double *outKernelMs, int *outCalls, long long *outEvaluations);

/* ---- multi-GPU, one process per GPU (MPI-style hosts; PhyML's MPI build runs one process per rank) -------------- */

/* ncclGetUniqueId: rank 0 calls it and broadcasts the PHYHIP_UNIQUE_ID_BYTES bytes by whatever means the host has (MPI_Bcast). */
int phyhip_comm_get_unique_id(char *outId);
/* ncclCommInitRank on the instance's device and stream.  The instance holds this rank's contiguous pattern shard (the
   caller slices its inputs); from now on phyhip_calculate_edge_log_likelihoods and phyhip_calculate_eigen_lnl[_dlnl]
   return the sum over ALL ranks on every rank (one all-reduce per evaluation, as for the sharded instance). */
int phyhip_comm_init_rank(int instance, int nranks, int rank, const char *uniqueId);
/* number of ranks in the instance's communicator(s) (1: no communicator) */
int phyhip_comm_size(int instance, int *outRanks);
/* pattern range and device of shard `shard` of an instance; returns the number of shards (1 for a plain instance) */
int phyhip_get_shard_range(int instance, int shard, int *outDevice, int *outFirstPattern, int *outPatternCount);

/* ---- stream / timing plumbing ---------------------------------------------------------------- */

/* Run on the caller's HIP stream (e.g. torch's current stream) instead of the instance's own. */
int phyhip_set_stream(int instance, void *hipStream);
int phyhip_synchronize(int instance);

/* Kernel timing with HIP events on the instance's stream, around the traversal kernel only.
   enable != 0 starts (and resets) accumulation. */
int phyhip_profile(int instance, int enable);
int phyhip_profile_read(int instance, double *outTraversalMs, int *outLaunches, double *outSiteUpdates);
/* The collective path of the evaluations profiled since phyhip_profile(instance, 1) on a sharded instance or on a rank of
   phyhip_comm_init_rank: HIP events on the first shard's stream around {per-device local sum, ncclAllReduce, publish kernel} --
   the time from this rank's traversal kernel having ended to the reduced scalar being on its way to the host, which includes
   waiting for the slowest rank.  outRanks: the communicator's size (1: no communicator, nothing measured). */
int phyhip_profile_read_collective(int instance, double *outMs, int *outCount, int *outRanks);
/* Name of the traversal kernel of the last launch profiled since phyhip_profile(instance, 1), template arguments included, as
   rocprofv3 --kernel-trace shows it without the namespace (bench.py: `roofline.kernel`); empty before the first such launch.
   Sharded instances: the first shard's. */
int phyhip_profile_read_kernel(int instance, char *outName, int capacity);
/* Traffic model of the launches profiled since phyhip_profile(instance, 1): the bytes those traversal launches had to
   move if nothing but the kernel's own register forwarding saved any -- every result written once, every child read
   unless it is a tip (1 byte) or one of the two previous results.  The honest floor under the algorithmic byte count of
   SURVEY 8(d), which also charges the forwarded reads. */
int phyhip_profile_read_traffic(int instance, double *outReadBytes, double *outWriteBytes);
/* The eigen-basis kernels launched since phyhip_profile(instance, 1): Update_Eigen_Lr's kernel (src/lk.c:1038) and the
   dLk / eigen-basis Lk kernel (src/lk.c:655-753), milliseconds and launches of each (HIP events on the instance's stream). */
int phyhip_profile_read_eigen(int instance, double *outEigenLrMs, int *outEigenLrLaunches, double *outDlkMs, int *outDlkLaunches);
/* The kernel of phyhip_calculate_node_state_posteriors while the instance is being profiled: milliseconds (HIP events on the
   instance's stream, uploads and the download of the result excluded) and calls since the previous read; reading resets both.
   Sharded instances: added over the shards. */
int phyhip_profile_read_node_posteriors(int instance, double *outKernelMs, int *outCalls);
/* The kernels of phyhip_calculate_pairwise_ml_distances while the instance is being profiled: milliseconds of the count kernels
   (shard sums and the per-pair sums included) and of the optimiser kernels (HIP events on the instance's stream; the host's
   starting values and the transfers excluded), and calls since the previous read; reading resets all three. */
int phyhip_profile_read_pairwise(int instance, double *outCountMs, double *outOptimiseMs, int *outCalls);
/* The kernels of phyhip_calculate_sh_support while the instance is being profiled (table, totals, draws, count): milliseconds (HIP
   events on the instance's stream; the host's alias table and the transfers excluded) and calls since the previous read; reading
   resets both. */
int phyhip_profile_read_support(int instance, double *outKernelMs, int *outCalls);

/* The resident evaluators (small nucleotide alignments, scalar wanted on the host): the launch-bound calls of a search --
   the chain of dLk calls of a branch-length optimisation (src/optimiz.c: Br_Len_Opt) and the short evaluations of SPR
   (src/spr.c:643-646: up to four matrices rebuilt, one or two partial updates, the edge likelihood) -- are served by
   workgroups that stay on the device and take each evaluation from a host-mapped command record instead of a kernel
   launch per call, whenever nothing else of the instance is known to be running on its stream.  Counters since the
   instance was created, out[0..3] for the dLk evaluator and out[4..7] for the short-evaluation one: evaluations served that
   way, launches of the resident workgroups, commands nobody answered (the evaluation was then launched the ordinary way),
   evaluations launched the ordinary way because work queued on the stream was not known to have finished.
   PHYHIP_RESIDENT=0 in the environment switches both off; PHYHIP_RESIDENT_IDLE_US (default 1000) is how long the workgroups
   wait for a command before they leave. */
int phyhip_get_resident_stats(int instance, long long out[8]);

/* The same four counters for the large-grid resident evaluator (phyml_amd/csrc/phyhip_big.hpp): nucleotide instances of more
   than 64 pattern tiles (~2 000 patterns) whose scalar-returning calls -- SPR candidates, Lk(b), Update_Eigen_Lr, dLk -- are
   served by one persistent workgroup per compute unit instead of a launch per call.  One instance per device at a time holds
   those workgroups; they leave when the instance launches anything else, or after PHYHIP_RESIDENT_IDLE_US without a command. */
int phyhip_get_big_resident_stats(int instance, long long out[4]);

/* Virtual buffers.  A tip x tip partial vector ("cherry": both children of the node are tips, src/avx.c:527-549 Exex) is two
   matrix columns and one product per pattern -- cheaper to recompute in registers than to write (C*S*8+4 bytes per pattern)
   and read back.  A traversal launch of at least `minOperations` operations therefore does not STORE such results when every
   reader of them sits later in the same launch: the defining operation is issued in front of each reader instead, its result
   forwarded in registers, and the buffer's memory stays stale ("virtual").  Whatever reads such a buffer later -- a queued
   operation, an evaluation edge, phyhip_update_eigen_lr, phyhip_get_partials / _scale_factors, a mixture evaluation -- first
   gets the defining operation queued again, storing: every value that leaves through this interface is the double the reference
   has in t_edge::p_lk_* at that point (tests/test_gpu_virtual.py).  A matrix or tip row the definition reads cannot change
   under it: before one changes, its old value is moved to a snapshot slot of the buffer (whole-tree batches of device-built
   matrices, uploaded matrices) or the dependants are stored first.  Only launches of the list form take part (at least three operations stay in the launch, whatever
   minOperations says).  minOperations = 0 switches the feature off (and stores what
   is virtual); the default is 16, so the short launches of a tree search never leave anything virtual -- and the first of
   them that reads a virtual buffer stores them all, in its own launch.  Not on class-axis or generic-loop instances.  Sharded
   instances: applied to every shard.
     The same launches leave a second class of result unstored, "deferred": a result of any operation that every reader in the
   launch takes from registers (the next two operations) and whose children are tips or buffers the launch leaves in memory.
   Nothing is recomputed for it -- the operation runs at its place, only its store goes -- and its definition is that one
   operation over stored inputs.  Everything above holds for it: the same readers store it first, the same snapshot slots keep its
   matrices, the first short launch that reads one stores all of both classes, minOperations = 0 stores all of both classes and
   stops deferring.  In addition a later launch that writes the buffer before reading it drops the definition (every repeated
   whole-tree traversal does, for every deferred buffer: nothing is launched for it), and one that writes a buffer the definition
   reads -- or phyhip_set_partials / phyhip_set_scale_factors on it -- stores the dependant first, on the old content (a short
   launch that has to store one stores all of both classes with it, so that the short launches behind it keep their form). */
int phyhip_set_virtual_buffers(int instance, int minOperations);

/* out[0] buffers virtual right now, out[1] stores skipped so far (operations that left their result virtual), out[2] non-storing
   re-issues in front of readers, out[3] storing re-issues (materialisations).  Sharded instances: the first shard's counters. */
int phyhip_get_virtual_stats(int instance, long long out[4]);

/* The deferred class (phyhip_set_virtual_buffers): out[0] buffers deferred right now, out[1] stores deferred so far, out[2]
   definitions stored on demand, out[3] definitions dropped because the buffer was written again first.  out[1] = out[0] + out[2] +
   out[3].  None of them counts in phyhip_get_virtual_stats.  Sharded instances: the first shard's counters. */
int phyhip_get_deferred_stats(int instance, long long out[4]);

/* Chained buffers: the third class of unstored result.  The deferred class keeps a forwarded result stored whenever one of its
   children is itself unstored, and a post-order is mostly chains (tip x cherry, then the result of the step before), so most
   forwarded results stay stored only so that a later reader could find them in memory.  A launch of the list form with at least
   `minOperations` operations (default 16; 0: off) in which NO TRANSITION MATRIX IS READ TWICE -- a one-sided traversal, the
   Lk(NULL) that Generic_Brent_Lk repeats while a model parameter is optimised -- leaves such a result unstored as well: a child
   may be a tip, a buffer in memory, or a buffer that is unstored after the launch (virtual, deferred, or chained earlier in the
   list).  Nothing is recomputed inside the launch and no kernel differs; the stores go.  Both-sided traversals (post-order and
   pre-order share the edge matrices) and the short launches of a search never chain.
     The cost side: a chained definition is one step of a recursion, not one step over stored inputs.  Every definition of any
   class carries a sequence number (inputs lower than dependants), and whatever stores a chained buffer -- the readers listed
   above, the setters, a matrix without a free snapshot slot, a tip row -- stores its unstored inputs with it, transitively, in
   that order, in front of the queue.  The first read of a buffer deep in a tree behind a one-sided traversal therefore launches up
   to the whole traversal once more, storing ("a short launch that has to store one stores all": at most one all-stored traversal,
   once); a repeated traversal launches nothing for the old definitions.  A later launch settles what earlier ones left, for the
   deferred and the chained class by one rule: definitions whose buffer it reads first, or whose input buffer it writes while the
   buffer itself stays, are stored in front together with their unstored inputs; definitions whose buffer it writes first are
   dropped unless one of those needs them; the rest stays.  phyhip_set_virtual_buffers(0) stores all three classes and stops
   all three; another threshold there does not move this one.  Values that leave through this interface are unchanged
   (tests/test_gpu_chained.py).  Sharded instances: applied to every shard. */
int phyhip_set_chained_buffers(int instance, int minOperations);

/* The chained class: out[0] buffers chained right now, out[1] stores left out so far, out[2] definitions stored on demand, out[3]
   definitions dropped.  out[1] = out[0] + out[2] + out[3].  They count neither in phyhip_get_virtual_stats nor in
   phyhip_get_deferred_stats (a deferred or virtual input stored with a chained buffer counts in its own class).  Sharded
   instances: the first shard's counters. */
int phyhip_get_chained_stats(int instance, long long out[4]);

/* The operation records of the nucleotide list-form launches (4 states, up to 4 categories): out[0] lists built in the compact
   form, out[1] list-form launches that found their list in a device slot and built nothing.  Then, over the lists built, how an
   operation's child reaches its step -- out[2 + 5 * s + k], s = 0 / 1 the first / second child, k = 0 a tip row, 1 computed in the
   step (a virtual tip x tip result), 2 / 3 forwarded in registers from the previous / second-previous operation, 4 loaded from
   its buffer -- padding records of odd lists included.  Sharded instances: the first shard's counters. */
int phyhip_get_record_stats(int instance, long long out[12]);

/* The step kinds of the compact lists built so far: out[8 * parity + kind], parity = the step's number in its list modulo 2
   (the kernel's loop body holds an even and an odd step), padding records included.  Kind 0 is the generic step; 1 tip x
   forwarded k-1, 2 forwarded k-1 x tip, 3 in-step x forwarded k-1, 4 forwarded k-1 x in-step, 5 in-step x tip, 6 tip x in-step,
   7 unused.  A step gets a kind other than 0 only if every tip row it reads (an in-step child's two included) is one-hot
   throughout.  Sharded instances: the first shard's counters. */
int phyhip_get_step_kind_stats(int instance, long long out[16]);

/* What the instance keeps per nucleotide tip row, computed from n state-set bytes: bit 0 every code is one-hot (1, 2, 4 or 8),
   bit 1 some code is 15.  Host arithmetic only: needs no device. */
int phyhip_tip_row_bits(const unsigned char *codes, long long n);

/* ---- parsimony (src/pars.c) --------------------------------------------------------------------------------------------------- */

/* Update_Partial_Pars (src/pars.c:239-393) and Pars / Pars_Core (src/pars.c:20-52, 397-437) on the device, in the reference's own
   integers: every value that leaves through these calls equals t_edge::ui_l/r, pars_l/r, p_pars_l/r, tree->site_pars, tree->c_pars.
   Parsimony buffers share the index space of the partials buffers: k < tipCount is tip k -- read from the tip data the instance
   already holds (the reference's Init_Ui_Tips / Init_Partial_Pars_Tips run the likelihood's character encoders), so a tip rewrite
   is seen in stream order -- and k >= tipCount is the parsimony plane that goes with partials buffer k.  Planes exist once
   phyhip_set_parsimony was called, and only for the mode in use: Fitch (general == 0: {ui, pars}, 8 bytes per pattern and buffer)
   or the step matrix (general != 0: stateCount ints per pattern and buffer).
   The parsimony queue is its own: none of these calls launches a queued likelihood operation, writes partials, scale vectors,
   matrices, site outputs or the warning flag, or counts as a step for the resident evaluators.  4 and 20 states.  Sharded
   instances of one process: every shard runs its pattern range, the host adds the 64-bit sums, per-pattern downloads are
   concatenated.  Not built (PHYHIP_ERROR_NO_IMPLEMENTATION): ranks of phyhip_comm_init_rank, class-axis instances, mixture trees
   (MIXT_Pars).  Every check happens before any device work: a call before phyhip_set_parsimony PHYHIP_ERROR_UNINITIALIZED_INSTANCE;
   a buffer index out of range, a destination that is a tip or one of its own children PHYHIP_ERROR_OUT_OF_RANGE. */
typedef struct { int destination, child1, child2; } phyhip_parsimony_operation;

/* enable parsimony; general != 0 needs stepMatrix[S*S] (row = parent state: tree->step_mat of Get_Step_Mat, the caller's own), else it
   may be NULL; re-callable (what is queued runs first in the mode it was queued in; a mode switch frees the other mode's planes) */
int phyhip_set_parsimony(int instance, int general, const int *stepMatrix);
/* queue operations (no launch); executed in order by the next calculate/get/synchronize, or when the staging list is full */
int phyhip_update_partial_parsimony(int instance, const phyhip_parsimony_operation *ops, int count);
/* flush the queue and score the edge whose two sides are these buffers (either may be a tip) in the SAME launch; count may have been
   0.  *outParsimony = sum over patterns of site_pars * weight, exact in 64 bits; a weight that is not an integer:
   PHYHIP_ERROR_NO_IMPLEMENTATION and nothing runs (the reference's c_pars += site_pars * wght truncates a double into an int at
   every pattern, in order).  outParsimony == NULL: the queue and the per-pattern scores only, whatever the weights -- the caller
   forms its own sum from phyhip_get_site_parsimony. */
int phyhip_calculate_edge_parsimony(int instance, int buffer1, int buffer2, long long *outParsimony);
int phyhip_get_site_parsimony(int instance, int *outSitePars);                       /* of the last scored edge */
/* flushes the queue; Fitch mode fills outUi / outPars [pattern], the step-matrix mode outPPars [pattern][state]; any may be NULL, one
   the mode does not hold PHYHIP_ERROR_OUT_OF_RANGE */
int phyhip_get_partial_parsimony(int instance, int bufferIndex, int *outUi, int *outPars, int *outPPars /* [pattern][state] */);
/* while phyhip_profile(instance, 1): milliseconds of the parsimony kernels (HIP events on the instance's stream), their launches and
   pattern x (operations + scored edges) since the previous read; reading resets all three.  Sharded: the slowest shard's time. */
int phyhip_profile_read_parsimony(int instance, double *outKernelMs, int *outLaunches, double *outPatternUpdates);

/* K regraft candidates of Spr_Pars in ONE call (src/spr.c:639-651 with spr_pars == YES: Graft_Subtree, Update_Partial_Pars(b_arrow,
   n_link), Pars(b_arrow), Prune_Subtree for every target edge of a pruned subtree).  Candidate k, in the mode in use: J = the join of
   child1 and child2 as Update_Partial_Pars forms it (src/pars.c:380-391, :359-375) -- never stored --, site[p] = Pars_Core of the edge
   (J, subtree) (:411-433), outParsimony[k] = sum over patterns of site[p] * weight[p], exact in 64 bits.  Indices as above: below
   tipCount a tip, else the plane of that buffer; child1 == child2 is allowed.
   Unlike the six calls above, a scan is a call that puts work on the stream: it enters as the other candidate-list calls do (a
   sharded instance's recorded calls drain, the large-grid resident workgroups leave).  Operations queued by
   phyhip_update_partial_parsimony run first, in stream order (the path updates of Test_One_Spr_Target_Recur, src/spr.c:545), and
   count as launches of phyhip_profile_read_parsimony like any other flush; the scan's own kernels do not.  Nothing else of the
   instance changes but the call's work space (24 bytes a candidate and 8 per tile of 256 patterns, the kept plane and the kept site
   scores) and its profile
   counters: the planes, the site scores of the last scored edge and everything on the likelihood side stay.  A result depends on
   the candidate alone -- not on count, its place in the list, the chunks (65535 candidates each) or the grid.  count == 0 succeeds.
   keepCandidate (-1: none) keeps J and site[] of one candidate for the two getters below, whose shapes and mode rules are those of
   phyhip_get_partial_parsimony; they return PHYHIP_ERROR_OUT_OF_RANGE before any scan, after a scan with -1, after a mode switch
   through phyhip_set_parsimony, or for an array the mode does not hold.
   Refused before any device work of any shard: what the parsimony calls refuse by kind of instance, and a call before
   phyhip_set_parsimony; an index out of range, keepCandidate outside -1 .. count - 1, a NULL array with count > 0
   (PHYHIP_ERROR_OUT_OF_RANGE); a pattern weight that is not an integer (PHYHIP_ERROR_NO_IMPLEMENTATION, as the edge call).
   Sharded instances of one process: every shard scans its pattern range, the host adds the integer sums, the kept vectors are
   concatenated.  Not built: mixture trees (MIXT_Pars). */
typedef struct { int child1, child2, subtree; } phyhip_parsimony_candidate;
int phyhip_calculate_regraft_parsimony(int instance, const phyhip_parsimony_candidate *candidates, int count, int keepCandidate,
                                       long long *outParsimony /* [count] */);
int phyhip_get_regraft_site_parsimony(int instance, int *outSitePars /* [pattern] */);
int phyhip_get_regraft_partial_parsimony(int instance, int *outUi, int *outPars, int *outPPars /* [pattern][state] */);
/* while phyhip_profile(instance, 1): milliseconds of the scan kernels, the calls and the candidates they served since the previous
   read; reading resets all three.  Sharded: the time is added over the shards. */
int phyhip_profile_read_regraft_parsimony(int instance, double *outKernelMs, int *outCalls, long long *outCandidates);

/* ---- regraft scan (src/spr.c: Test_One_Spr_Target) ------------------------------------------------------------------------------ */

/* K regraft candidates of one pruned subtree in ONE call.  Candidate k joins three vectors that exist already: outLogLikelihoods[k] is
   what phyhip_update_partials {destination a spare buffer, child 1 through the matrix of child1Length, child 2 through the matrix of
   child2Length} followed by phyhip_calculate_edge_log_likelihoods {parent that spare buffer, child subtreePartials, the matrix of
   subtreeLength} returns -- with PHYHIP_REGRAFT_SUBTREE_IS_LEFT the operands swap: the subtree is the parent operand and the computed
   vector the child (subtreePartials must then be a partials buffer: a left side is never a tip in PhyML).  An index below tipCount
   is a tip.  The three matrices of a candidate are built inside the call, into the unit's work space, from eigen system eigenIndex
   with exactly the treatment phyhip_update_transition_matrices gives a length (MAX(0, l) x rate x br_len_mult, the clamp, the
   SMALL_PIJ floor, the row renormalisation; the reference libm's exp): they are the reference's doubles, and so is the computed
   vector (Exex / Exin / Inin by kind of child, the all-ones shortcut, patterns of weight <= DBL_MIN skipped, the children's
   exponents added, the 2^256 rule under apply_lk_scaling).  The evaluation is Lk_Core's (the general product at every pattern,
   Pull_Scaling_Factors, the category mix, Invariant_Lk's +I mix, the SMALL floor with its warning, the reference libm's log): the
   reference's lnL to ~1e-13 relative, like phyhip_calculate_edge_log_likelihoods.  The bits of outLogLikelihoods[k] depend on
   candidate k alone -- not on count, on k's place in the list or on how the call was cut into chunks (no floating-point atomics:
   lane, wave, tile sums added in one fixed order).
     State: queued matrix work and queued partial updates run first (the path updates of Test_One_Spr_Target_Recur, queued with
   phyhip_update_partials, are seen); virtual buffers a candidate names are stored; then NOTHING of the instance changes but this
   unit's work space -- every partial and scale vector, the matrix table, the per-site outputs, dot_prod and the numerical warning
   stay as they were.  outWarnings[k] (may be NULL) is candidate k's own warning.  keepCandidate (-1: none) names one candidate whose
   computed vector and scale vector are also kept in the work space for phyhip_get_regraft_partials; a caller that wants them in
   a buffer uploads them (phyhip_set_partials / phyhip_set_scale_factors).  A plain call: the large-grid resident workgroups leave;
   it waits for the stream and leaves it clean, so the Lk(b) / dLk calls that follow are served resident again.
     Work space: 3 C S S doubles, one double per tile of 256 patterns and 72 bytes per candidate, next to the kept vector
   (P C S doubles and P ints), grown on use, kept on the instance and bounded by phyhip_set_regraft_work_space (0: the default of
   128 MiB); a list that needs more runs in chunks of candidates (at least one per chunk).  Identical lengths of a chunk are built
   once.
     One-process sharded instances: every shard scans its pattern range, the host adds each candidate's shard sums in shard order,
   the kept vector is concatenated.  count == 0 succeeds and does nothing.  Not built (PHYHIP_ERROR_NO_IMPLEMENTATION): ranks of
   phyhip_comm_init_rank, PHYHIP_FLAG_CLASS_AXIS and PHYHIP_FLAG_GENERIC_LOOP instances, states other than 4 / 20, MORE THAN 8
   CATEGORIES (the 4-state kernel holds C x 4 values in registers; such instances are refused, not served).  A mixture's class
   instances are scanned together by phyhip_calculate_mixture_regraft_log_likelihoods, below.
   PHYHIP_ERROR_OUT_OF_RANGE: a buffer, tip or eigen index out of range, a tip as the left operand, keepCandidate >= count. */
#define PHYHIP_REGRAFT_SUBTREE_IS_LEFT 1
typedef struct
{
  int    child1Partials;   /* partials buffer or tip index: one side of the target edge        */
  int    child2Partials;   /* ... the other side                                                */
  int    subtreePartials;  /* the pruned subtree's vector: partials buffer or tip               */
  int    flags;
  double child1Length, child2Length, subtreeLength;  /* b->l->v of the two halves and of b_arrow */
} phyhip_regraft_candidate;

int phyhip_calculate_regraft_log_likelihoods(int instance, int eigenIndex, const phyhip_regraft_candidate *candidates,
                                             int count, int keepCandidate, double *outLogLikelihoods, int *outWarnings);
/* of keepCandidate of the last call: [pattern][category][state] and [pattern] (either may be NULL; rows of patterns without weight
   are zero).  Before any call, or after one with keepCandidate -1: PHYHIP_ERROR_OUT_OF_RANGE */
int phyhip_get_regraft_partials(int instance, double *outPartials, int *outScaleFactors);
/* matrix `which` (0 child 1, 1 child 2, 2 subtree) of candidate `candidate` of the last call as the scan read it, [category][from][to].
   A call that ran in chunks keeps the LAST chunk's matrices: an earlier candidate, a `which` outside 0..2 or a call before any scan:
   PHYHIP_ERROR_OUT_OF_RANGE */
int phyhip_get_regraft_transition_matrix(int instance, int candidate, int which, double *outMatrix);
/* bound on the unit's work space in bytes (0: the default, 128 MiB) */
int phyhip_set_regraft_work_space(int instance, long long maxBytes);
/* while phyhip_profile(instance, 1): milliseconds of the matrix, scan and sum kernels (HIP events on the instance's stream; uploads
   and downloads excluded; sharded: added over the shards), the calls and the candidates they served since the previous read;
   reading resets all three */
int phyhip_profile_read_regraft(int instance, double *outKernelMs, int *outCalls, long long *outCandidates);

/* ---- regraft scan of a mixture (src/spr.c: Test_One_Spr_Target on a mixture tree: MIXT_Update_Partial_Lk, MIXT_Lk) -------------- */

/* K regraft candidates of one pruned subtree over ALL class trees of a mixture in ONE call.  instances[count] are the class
   instances (one category each, as phyhip_calculate_mixture_log_likelihood takes them; 1..64), eigenIndices[count] the eigen system
   each class takes; classProba / rMatWeight / eFrqWeight [count] and the three sums are MIXT_Lk's coefficients.  The class trees
   share topology and buffer numbering, so ONE record serves every class: a record's buffer and tip indices mean the same buffer in
   every class instance, and its three lengths are the mixture tree's -- each class scales them by its own category rate and
   br_len_mult and clamps with its own l_min / l_max, exactly as phyhip_update_transition_matrices does for that instance.
   outLogLikelihoods[k] is what the per-candidate route returns: in every class instance phyhip_update_transition_matrices of the
   three lengths and phyhip_update_partials {a spare buffer <- child 1, child 2}, then ONE phyhip_calculate_mixture_log_likelihood
   over the class list {that spare buffer, subtreePartials, the third matrix} (PHYHIP_REGRAFT_SUBTREE_IS_LEFT: the operands swap).
     Per class everything phyhip_calculate_regraft_log_likelihoods does for an instance of one category: the three matrices built
   into the work space (the reference's doubles), the joined vector as AVX_Update_Partial_Lk would store it (the reference's doubles:
   tips from the class instance's own tip data, the all-ones shortcut, patterns of weight <= DBL_MIN skipped, the children's
   exponents added, the 2^256 rule), Lk_Core's product with the subtree: the class likelihood x_k and the exponent f_k its own edge
   evaluation would leave in unscaled_site_lk_cat / fact_sum_scale.  Then the site loop of MIXT_Lk (src/mixt.c:1027-1142) in the
   operation order of phyhip_calculate_mixture_log_likelihood: f_k > 1024 becomes 1023 and raises the candidate's warning, a class at
   exactly 1024 drops out, site_lk += x * proba * r_w / r_sum * e_w / e_sum / sum_probas in class order, the +I share set with
   phyhip_set_mixture_invariant_sites on the FIRST instance, the SMALL floor with the candidate's warning, the reference libm's log,
   the FIRST instance's pattern weights; a pattern without weight adds nothing.  The reference's lnL to ~1e-13 relative.  The bits of
   outLogLikelihoods[k] depend on candidate k and the class list alone -- not on candidateCount, on k's place in the list or on the
   chunks (no floating-point atomics: lane, wave, tile sums added in one fixed order); another order of the classes is another sum.
     State: in every class instance queued matrix work and queued partial updates run first and virtual buffers a record names are
   stored, all of it before anything is launched; the kernels run on the first instance's stream; the call waits for it and leaves
   every class stream clean (the large-grid resident workgroups leave; Lk(b) / dLk afterwards are served resident again).  NOTHING
   of any instance changes but a work space kept on the FIRST instance, apart from the plain scan's own: partials, exponents, matrix
   tables, site outputs, dot_prod and warning flags stay as they were.  outWarnings[k] (may be NULL) is candidate k's own warning.
   keepCandidate (-1: none): that candidate's computed vector and exponents are kept for every class.
     Work space: per candidate 3 S S doubles a class, one double per tile of 256 patterns and 72 bytes; next to them the kept vectors
   (P S doubles and P ints a class) and the per-class table (128 bytes a class, uploaded with the records); grown on use, bounded by
   phyhip_set_mixture_regraft_work_space (0: the default of 128 MiB); a longer list runs in chunks of at least one candidate.
   Identical lengths of a chunk are built once per class.
     Class instances that are one-process sharded instances of one shard layout: every shard scans its pattern range over its
   sub-instances, the host adds each candidate's shard sums in shard order, the kept vectors are concatenated.  candidateCount == 0
   succeeds and does nothing.  PHYHIP_ERROR_OUT_OF_RANGE: count outside 1..64, an instance with more than one category, differing
   pattern counts, state counts, buffer layouts or devices, sharded and plain instances mixed, a bad buffer, tip or eigen index, a
   tip as the left operand, keepCandidate >= candidateCount.  Not built (PHYHIP_ERROR_NO_IMPLEMENTATION): class-axis entries,
   PHYHIP_FLAG_GENERIC_LOOP instances, ranks of phyhip_comm_init_rank, states other than 4 / 20. */
int phyhip_calculate_mixture_regraft_log_likelihoods(const int *instances, int count, const int *eigenIndices,
                                                     const phyhip_regraft_candidate *candidates, int candidateCount, int keepCandidate,
                                                     const double *classProba, const double *rMatWeight, const double *eFrqWeight,
                                                     double rMatWeightSum, double eFrqWeightSum, double sumProbas,
                                                     double *outLogLikelihoods, int *outWarnings);
/* of keepCandidate of the last call with this first instance, class classIndex: [pattern][state] and [pattern] (either may be NULL;
   rows of patterns without weight are zero).  Before any call, after one with keepCandidate -1, or a class that is not there:
   PHYHIP_ERROR_OUT_OF_RANGE */
int phyhip_get_mixture_regraft_partials(int firstInstance, int classIndex, double *outPartials, int *outScaleFactors);
/* matrix `which` (0 child 1, 1 child 2, 2 subtree) of class classIndex and candidate `candidate` of the last call as the scan read
   it, [from][to].  A call that ran in chunks keeps the LAST chunk's matrices: an earlier candidate, a class or candidate that is not
   there, a `which` outside 0..2 or a call before any scan: PHYHIP_ERROR_OUT_OF_RANGE */
int phyhip_get_mixture_regraft_transition_matrix(int firstInstance, int classIndex, int candidate, int which, double *outMatrix);
/* bound on the work space in bytes (0: the default, 128 MiB) */
int phyhip_set_mixture_regraft_work_space(int firstInstance, long long maxBytes);
/* while phyhip_profile(firstInstance, 1): milliseconds of the matrix, scan and sum kernels (HIP events on the first instance's
   stream; uploads and downloads excluded; sharded: added over the shards), the calls and the candidates they served since the
   previous read; reading resets all three */
int phyhip_profile_read_mixture_regraft(int firstInstance, double *outKernelMs, int *outCalls, long long *outCandidates);

/* ---- three-edge length search (src/utilities.c:7120-7146: Triple_Dist) ------------------------------------------------------------- */

/* Triple_Dist at K internal nodes in ONE call.  A candidate is a node a with its three OUTER vectors -- partials[i] is the vector
   that looks AT the node along a->b[i] (a partials buffer, or a tip index < tipCount), which Triple_Dist never changes -- and the
   three lengths a->b[i]->l->v.  Per candidate, one workgroup of one plain launch runs (phyml_amd/csrc/phyhip_triple.hip):
     the matrices of the three lengths (PMat_Empirical as phyhip_update_transition_matrices builds them); then for i = 0, 1, 2
       I_i      Update_Partial_Lk(tree, a->b[i], a): the join of the two other outer vectors through their current matrices in
                ascending edge order -- (1,2), (0,2), (0,1) -- with its exponents, as the regraft scan computes it;
       lkBegin  Br_Len_Opt's Lk(b[i]): Lk_Core through matrix i between I_i and partials[i].  PHYHIP_TRIPLE_NODE_IS_LEFT(i) says
                that a is b[i]->left -- I_i is the LEFT operand; clear, partials[i] is, and must then be an internal buffer.
                Summed in one fixed order: a thread's patterns in ascending order (pattern = thread + round * threads), the
                wave's shuffle-down tree 32..1, the waves in wave order;
       the eigen-basis products and per-pattern exponents of that edge (phyhip_update_eigen_lr's arithmetic), into the work space;
       the search of phyhip_optimise_edge_length from (length[i], lkBegin): the same steps, the same per-pattern terms;
       length[i] = best_l, matrix i rebuilt, and Br_Len_Opt's check lk_end < lk_begin - tol (src/optimiz.c:656): status 8.
     A status of 3..8 is where the reference stops the program: the candidate stops there and its later searches report -1.
     length[i] of the search that stopped is its best_l so far (what the host-driven search leaves in *l; matrix i is NOT rebuilt),
     lnL / dLnL are that search's; the lengths of the edges not reached are the inputs.
     keepCandidate (-1: none): I_1 and I_0 are rebuilt from the final lengths (:7141-7142) and kept with the final I_2 for
     phyhip_get_triple_partials (host order [pattern][category][state], and the exponents [pattern]); entries of a pattern without
     weight are 0.  Nothing is kept of a candidate that stopped.
   The bits of a candidate's result depend on the candidate alone: not on K, its place in the list or the chunks a bounded work
   space (phyhip_set_triple_work_space; 0: the default of 128 MiB; per candidate 3 C S S + P C S doubles and P ints, and the three
   kept vectors once) cuts the call into.
     A plain call: queued matrix work and partial updates run first, virtual buffers a candidate names are stored, the large-grid
   resident workgroups leave, the call waits for the stream and leaves it clean.  Nothing of the instance changes but this work
   space and the numerical warning (the last candidate's last evaluation's): not partials, exponents, the matrix table, site outputs
   or dot_prod.
     Not built (PHYHIP_ERROR_NO_IMPLEMENTATION, nothing launched; the caller runs Triple_Dist edge by edge): ranks of
   phyhip_comm_init_rank, one-process sharded instances, PHYHIP_FLAG_CLASS_AXIS and PHYHIP_FLAG_GENERIC_LOOP instances, more than
   one eigen system, states other than 4 / 20, more than 8 categories, more than 16 384 patterns.  A NaN length:
   PHYHIP_ERROR_FLOATING_POINT.  iterMax outside 1 .. 1000, tol <= 0, an index out of range, a tip without its flag, count < 0,
   keepCandidate outside -1 .. count - 1: PHYHIP_ERROR_OUT_OF_RANGE.  count == 0 succeeds. */
#define PHYHIP_TRIPLE_NODE_IS_LEFT(i) (1 << (i))
typedef struct
{
  int    partials[3];
  int    flags;
  double length[3];
} phyhip_triple_candidate;
typedef struct
{
  double length[3];                 /* on return */
  double lnL, dLnL;                 /* tree->c_lnL / c_dlnL as Triple_Dist leaves them: the last search's that ran */
  double lkBegin[3];                /* Br_Len_Opt's lk_begin of each search */
  int    evaluations[3], status[3]; /* phyhip_optimise_edge_length's statuses; -1: not reached; 8: lk_end < lk_begin - tol */
  int    warning;                   /* the last evaluation's */
  int    reserved;
} phyhip_triple_result;
int phyhip_optimise_triples(int instance, const phyhip_triple_candidate *candidates, int count, int iterMax, double tol,
                            int keepCandidate, phyhip_triple_result *outResults);
/* I_which (0..2) of the kept candidate of the last call: outPartials [pattern][category][state], outScaleFactors [pattern]; either
   may be NULL.  No call before it, no kept candidate, or one that stopped: PHYHIP_ERROR_OUT_OF_RANGE */
int phyhip_get_triple_partials(int instance, int which, double *outPartials, int *outScaleFactors);
/* bound on the work space in bytes (0: the default, 128 MiB); a longer list runs in chunks of at least one candidate */
int phyhip_set_triple_work_space(int instance, long long maxBytes);
/* while phyhip_profile(instance, 1): milliseconds of the kernel (HIP events on the instance's stream), the calls and the
   evaluations their searches took since the previous read; reading resets all three */
int phyhip_profile_read_triples(int instance, double *outKernelMs, int *outCalls, long long *outEvaluations);

#ifdef __cplusplus
}
#endif
#endif /* PHYHIP_H */
