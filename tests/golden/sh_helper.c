/*
 * sh_helper.c -- TEST INFRASTRUCTURE, compiled by tests/golden/make_sh.py into a temporary directory against
 * oracle/_ref/libphyml_ref.so (the real reference, built from its sources where they exist).  This repository's own code: it only
 * CALLS the reference's public functions, in the order of its program entry (src/main.c, as oracle/ref_driver.c does), then what
 * aLRT() runs in front of its edge loop (src/alrt.c:202-208: Set_Both_Sides(YES), Lk(NULL), Update_Dirs), then per internal edge
 * NNI_Neigh_BL, srand(edge number), Statistics_To_SH, Statistics_to_RELL -- and prints what tests/golden/sh_support_<case>.npz holds.
 * Then, for four weight vectors, srand(1) + 4096 raw rand() values and srand(1) + the 2048 indices Sample_n_i_With_Proba_pi returns.
 * Every double is printed with %a (exact).
 *
 * usage: sh_helper <phyml command line>
 */
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "utilities.h"
#include "lk.h"
#include "models.h"
#include "io.h"
#include "init.h"
#include "free.h"
#include "alrt.h"
#include "stats.h"
#include "spr.h"
#include "pars.h"
#include "make.h"

phydbl Statistics_to_RELL(t_tree *tree); /* src/alrt.c:1091: defined there, declared in no header of the reference */

static void vec(const char *name, const double *v, int n)
{
  printf("%s %d", name, n);
  for (int i = 0; i < n; ++i) printf(" %a", v[i]);
  printf("\n");
}

static double now(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

#define N_RAND 4096
#define N_DRAW 2048

int main(int argc, char **argv)
{
  option *io = (option *)Get_Input(argc, argv);
  if (!io) return 2;
  srand(io->r_seed < 0 ? 1 : io->r_seed);
  io->n_trees = 1;
  Get_Seq(io);
  Make_Model_Complete(io->mod);
  Set_Model_Name(io->mod);
  t_mod  *mod   = io->mod;
  calign *cdata = Compact_Data(io->data, io);
  Free_Seq(io->data, cdata->n_otu);
  Init_Model(cdata, mod, io);
  Set_Model_Parameters(mod);
  t_tree *tree = Dist_And_BioNJ(cdata, mod, io);
  if (!tree) return 3;
  tree->mod = mod; tree->io = io; tree->data = cdata;
  tree->n_root = NULL; tree->e_root = NULL; tree->n_tot_bl_opt = 0;
  Set_Both_Sides(YES, tree);
  Connect_CSeqs_To_Nodes(tree->data, tree->io, tree);
  Make_Tree_For_Pars(tree);
  Make_Tree_For_Lk(tree);
  Make_Spr(tree);
  Br_Len_Not_Involving_Invar(tree);
  Unscale_Br_Len_Multiplier_Tree(tree);
  Set_Update_Eigen(YES, tree->mod);
  Lk(NULL, tree);
  Set_Update_Eigen(NO, tree->mod);

  /* src/alrt.c:202-208 */
  Set_Both_Sides(YES, tree);
  Lk(NULL, tree);
  Update_Dirs(tree);

  const int P = cdata->n_pattern;
  printf("\nSH_BEGIN\n");
  printf("dims 3 %d %d %d\n", cdata->n_otu, P, cdata->init_len);
  vec("wght", cdata->wght, P);
  for (int i = 0; i < 2 * tree->n_otu - 3; ++i)
  {
    t_edge *b = tree->a_edges[i];
    if (b->left->tax || b->rght->tax) continue;
    NNI_Neigh_BL(b, tree);
    char nm[32];
    for (int k = 0; k < 3; ++k)
    {
      snprintf(nm, sizeof nm, "lks_%d_%d", i, k);
      vec(nm, tree->log_lks_aLRT[k], P);
    }
    srand((unsigned)i);
    const double t0 = now();
    const double sh = Statistics_To_SH(tree);
    const double t1 = now();
    const double rell = Statistics_to_RELL(tree);
    const double t2 = now();
    const double st[5] = {sh, rell, t1 - t0, t2 - t1, (double)i};
    snprintf(nm, sizeof nm, "stat_%d", i);
    vec(nm, st, 5);
    fflush(stdout);
  }

  /* the alias sampler against its own rand() stream, four weight vectors */
  double *w = (double *)malloc(sizeof(double) * P), *pi = (double *)malloc(sizeof(double) * P), *r = (double *)malloc(sizeof(double) * N_RAND);
  for (int v = 0; v < 4; ++v)
  {
    for (int i = 0; i < P; ++i)
    {
      if (v == 0) w[i] = cdata->wght[i];
      else if (v == 1) w[i] = 1.0;                                             /* every column "large" */
      else if (v == 2) w[i] = (double)(((unsigned)i * 2654435761u >> 13) % 4u); /* bootstrap-like, a quarter zeros */
      else w[i] = i == P / 3 ? 5.0 * P : 1.0;                                   /* one heavy pattern */
    }
    for (int i = 0; i < P; ++i) pi[i] = w[i] / (double)cdata->init_len;
    srand(1);
    for (int i = 0; i < N_RAND; ++i) r[i] = (double)rand();
    srand(1);
    int   *idx = Sample_n_i_With_Proba_pi(pi, P, N_DRAW);
    char   nm[32];
    double *d = (double *)malloc(sizeof(double) * N_DRAW);
    for (int i = 0; i < N_DRAW; ++i) d[i] = (double)idx[i];
    snprintf(nm, sizeof nm, "alias_w_%d", v);
    vec(nm, w, P);
    snprintf(nm, sizeof nm, "alias_rand_%d", v);
    vec(nm, r, N_RAND);
    snprintf(nm, sizeof nm, "alias_idx_%d", v);
    vec(nm, d, N_DRAW);
    free(d);
    Free(idx);
  }
  const double rm = (double)RAND_MAX;
  vec("rand_max", &rm, 1);
  printf("SH_END\n");
  return 0;
}
