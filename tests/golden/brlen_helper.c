/*
 * brlen_helper.c -- TEST INFRASTRUCTURE, compiled by tests/golden/make_brlen.py into a temporary directory against
 * oracle/_ref/libphyml_ref.so (the real reference, built from its sources where they exist).  This repository's own code: it only
 * CALLS the reference's public functions, in the order of its program entry (src/main.c, as oracle/ref_driver.c does, with that
 * driver's --gtr-rr option so that the committed .phyg files describe the same tree, model and data), then Set_Both_Sides(YES),
 * Lk(NULL), and for every edge and every start length  l0 * {1, 0.05, 20, 1e-6, 1e3} (capped at 90) and -l0:
 *     b->l->v = start;  lk_begin = Lk(b);  Br_Len_Opt(&b->l->v, b, tree);  one record;  b->l->v = l0;  Update_PMat_At_Given_Edge(b)
 * A record holds scalars only, every double printed with %a (exact): edge, start index, l_in, lk_begin, l_out, c_lnL, c_dlnL and
 * the growth of tree->n_tot_bl_opt.
 *
 * usage: brlen_helper [--gtr-rr a,b,c,d,e,f] -- <phyml command line>
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "utilities.h"
#include "lk.h"
#include "models.h"
#include "io.h"
#include "init.h"
#include "free.h"
#include "optimiz.h"
#include "spr.h"
#include "pars.h"
#include "make.h"

static const double FACTOR[6] = {1.0, 0.05, 20.0, 1e-6, 1e3, -1.0};

int main(int argc, char **argv)
{
  double rr[6];
  int    have_rr = 0, split = 0;
  for (int i = 1; i < argc; ++i)
  {
    if (!strcmp(argv[i], "--")) { split = i; break; }
    if (!strcmp(argv[i], "--gtr-rr") && i + 1 < argc)
    {
      if (sscanf(argv[++i], "%lf,%lf,%lf,%lf,%lf,%lf", rr, rr + 1, rr + 2, rr + 3, rr + 4, rr + 5) != 6) return 2;
      have_rr = 1;
    }
  }
  if (!split) return 2;
  argv[split] = argv[0];
  option *io = (option *)Get_Input(argc - split, argv + split);
  if (!io) return 2;
  srand(io->r_seed < 0 ? 1 : io->r_seed);
  io->n_trees = 1;
  Get_Seq(io);
  Make_Model_Complete(io->mod);
  Set_Model_Name(io->mod);
  t_mod *mod = io->mod;
  if (have_rr)
    for (int i = 0; i < 6; ++i) mod->r_mat->rr_val->v[i] = log(rr[i]);
  calign *cdata = Compact_Data(io->data, io);
  Free_Seq(io->data, cdata->n_otu);
  Init_Model(cdata, mod, io);
  if (have_rr)
    for (int i = 0; i < 6; ++i) mod->r_mat->rr_val->v[i] = log(rr[i]);
  Set_Model_Parameters(mod);
  t_tree *tree = io->in_tree == 2 ? Read_User_Tree(cdata, mod, io) : Dist_And_BioNJ(cdata, mod, io);
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

  Set_Both_Sides(YES, tree);
  Lk(NULL, tree);

  const int E = 2 * tree->n_otu - 3;
  printf("\nBRLEN_BEGIN\n");
  printf("dims %d %d %d\n", tree->n_otu, cdata->n_pattern, E);
  printf("opt %a %a %a %d\n", mod->l_min, mod->l_max, mod->s_opt->min_diff_lk_local, mod->s_opt->brent_it_max);
  printf("edge_len");
  for (int i = 0; i < E; ++i) printf(" %a", tree->a_edges[i]->l->v);
  printf("\n");
  for (int i = 0; i < E; ++i)
  {
    t_edge      *b = tree->a_edges[i];
    const double l0 = b->l->v;
    for (int k = 0; k < 6; ++k)
    {
      double lin = FACTOR[k] < 0.0 ? -l0 : l0 * FACTOR[k];
      if (lin > 90.0) lin = 90.0;
      b->l->v = lin;
      Set_Update_Eigen_Lr(NO, tree);
      Set_Use_Eigen_Lr(NO, tree);
      const double lk_begin = Lk(b, tree);
      const int    n0 = tree->n_tot_bl_opt;
      Br_Len_Opt(&(b->l->v), b, tree);
      printf("rec %d %d %a %a %a %a %a %d\n", i, k, lin, lk_begin, b->l->v, tree->c_lnL, tree->c_dlnL, tree->n_tot_bl_opt - n0);
      fflush(stdout);
      b->l->v = l0;
      Update_PMat_At_Given_Edge(b, tree);
    }
  }
  printf("BRLEN_END\n");
  return 0;
}
