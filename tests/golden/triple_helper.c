/*
 * triple_helper.c -- TEST INFRASTRUCTURE, compiled by tests/golden/make_triple.py into a temporary directory against
 * oracle/_ref/libphyml_ref.so (the real reference, built from its sources where they exist).  This repository's own code: it only
 * CALLS the reference's public functions, in the order of its program entry (src/main.c, as oracle/ref_driver.c and
 * tests/golden/brlen_helper.c do, with that driver's --gtr-rr option so that the committed .phyg files describe the same tree, model
 * and data), then Set_Both_Sides(YES), Lk(NULL), and for every internal node a and every scaling  {1, 0.05, 20}  of its three edges'
 * lengths (capped at 90):
 *     a->b[i]->l->v = l0[i] * scaling;  Triple_Dist(a, tree);  one record;  the three lengths restored;  Set_Both_Sides(YES);  Lk(NULL)
 * A record holds scalars only, every double printed with %a (exact): node, scaling index, the node's three edges, the three lengths
 * in and out, tree->c_lnL and the growth of tree->n_tot_bl_opt.
 *
 * usage: triple_helper [--gtr-rr a,b,c,d,e,f] -- <phyml command line>
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

static const double SCALING[3] = {1.0, 0.05, 20.0};

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
  printf("\nTRIPLE_BEGIN\n");
  printf("dims %d %d %d\n", tree->n_otu, cdata->n_pattern, E);
  printf("opt %a %a %a %d\n", mod->l_min, mod->l_max, mod->s_opt->min_diff_lk_local, mod->s_opt->brent_it_max);
  printf("edge_len");
  for (int i = 0; i < E; ++i) printf(" %a", tree->a_edges[i]->l->v);
  printf("\n");
  for (int n = tree->n_otu; n < 2 * tree->n_otu - 2; ++n)
  {
    t_node *a = tree->a_nodes[n];
    double  l0[3];
    for (int i = 0; i < 3; ++i) l0[i] = a->b[i]->l->v;
    for (int k = 0; k < 3; ++k)
    {
      double lin[3];
      for (int i = 0; i < 3; ++i)
      {
        lin[i] = l0[i] * SCALING[k];
        if (lin[i] > 90.0) lin[i] = 90.0;
        a->b[i]->l->v = lin[i];
      }
      const int n0 = tree->n_tot_bl_opt;
      Triple_Dist(a, tree);
      printf("rec %d %d %d %d %d %a %a %a %a %a %a %a %d\n", a->num, k, a->b[0]->num, a->b[1]->num, a->b[2]->num, lin[0], lin[1], lin[2],
             a->b[0]->l->v, a->b[1]->l->v, a->b[2]->l->v, tree->c_lnL, tree->n_tot_bl_opt - n0);
      fflush(stdout);
      for (int i = 0; i < 3; ++i) a->b[i]->l->v = l0[i];
      Set_Both_Sides(YES, tree);
      Lk(NULL, tree);
    }
  }
  printf("TRIPLE_END\n");
  return 0;
}
