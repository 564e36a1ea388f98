/*
 * pars_helper.c -- TEST INFRASTRUCTURE, compiled by tests/golden/make_pars.py into a temporary directory against
 * oracle/_ref/libphyml_ref.so (the real reference, built from its sources where they exist).  This repository's own code: it only
 * CALLS the reference's public functions, in the order of its program entry (src/main.c:148-236, as oracle/ref_driver.c does) up to
 * Make_Tree_For_Pars on the BioNJ tree or a user tree (-u), then, for general_pars = NO and YES (the toggle One_Pars_Step makes,
 * src/pars.c:448-458): Set_Both_Sides(YES), Pars(NULL), a dump of both sides of every edge, and Pars(b) for EVERY edge b -- and prints
 * what tests/golden/pars_<case>.npz holds.  Integers only.
 *
 * PARS_HELPER_TIME=<repeats> in the environment: additionally times Pars(NULL) with both sides, per mode, on the calling core and
 * prints nanoseconds per pattern-update (3(n-2) edge sides + the scored edge, times the pattern count).
 *
 * usage: pars_helper <phyml command line>
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
#include "pars.h"
#include "make.h"

static void ivec(const char *name, int a, int b, const int *v, int n)
{
  printf("%s_%d_%d %d", name, a, b, n);
  for (int i = 0; i < n; ++i) printf(" %d", v[i]);
  printf("\n");
}

static double now(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

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
  t_tree *tree = io->in_tree == 2 ? Read_User_Tree(cdata, mod, io) : Dist_And_BioNJ(cdata, mod, io);
  if (!tree) return 3;
  tree->mod = mod; tree->io = io; tree->data = cdata;
  tree->n_root = NULL; tree->e_root = NULL; tree->n_tot_bl_opt = 0;
  Set_Both_Sides(YES, tree);
  Connect_CSeqs_To_Nodes(tree->data, tree->io, tree);
  Make_Tree_For_Pars(tree);

  const int P = cdata->n_pattern, n = tree->n_otu, ns = mod->ns, E = 2 * n - 3;
  int *tmp = (int *)malloc(sizeof(int) * (size_t)(P > 3 * (2 * n - 2) ? P : 3 * (2 * n - 2)));
  printf("\nPARS_BEGIN\n");
  printf("dims_0_0 3 %d %d %d\n", n, P, ns);
  for (int e = 0; e < E; ++e) { tmp[2 * e] = tree->a_edges[e]->left->num; tmp[2 * e + 1] = tree->a_edges[e]->rght->num; }
  ivec("edges", 0, 0, tmp, 2 * E);
  for (int i = 0; i < 2 * n - 2; ++i)
    for (int k = 0; k < 3; ++k) tmp[3 * i + k] = tree->a_nodes[i]->v[k] ? tree->a_nodes[i]->v[k]->num : -1;
  ivec("node_v", 0, 0, tmp, 3 * (2 * n - 2));
  for (int i = 0; i < 2 * n - 2; ++i)
    for (int k = 0; k < 3; ++k) tmp[3 * i + k] = tree->a_nodes[i]->b[k] ? tree->a_nodes[i]->b[k]->num : -1;
  ivec("node_b", 0, 0, tmp, 3 * (2 * n - 2));
  const char *rep = getenv("PARS_HELPER_TIME");
  const int   timing = rep && atoi(rep) > 0; /* no dumps: only the times */
  for (int i = 0; i < n && !timing; ++i)
  {
    for (int s = 0; s < P; ++s) tmp[s] = (unsigned char)tree->a_nodes[i]->c_seq->state[s];
    ivec("seq", i, 0, tmp, P);
  }
  for (int s = 0; s < P; ++s)
  {
    tmp[s] = (int)cdata->wght[s];
    if ((double)tmp[s] != cdata->wght[s]) return 4;
  }
  ivec("wght", 0, 0, tmp, P);
  ivec("step_mat", 0, 0, tree->step_mat, ns * ns);

  for (int gp = 0; gp < 2; ++gp)
  {
    mod->s_opt->general_pars = gp;
    Set_Both_Sides(YES, tree);
    Pars(NULL, tree);
    for (int e = 0; e < E && !timing; ++e)
    {
      t_edge *b = tree->a_edges[e];
      if (!gp)
      {
        ivec("ui", e, 0, b->ui_l, P); ivec("ui", e, 1, b->ui_r, P);
        ivec("pars", e, 0, b->pars_l, P); ivec("pars", e, 1, b->pars_r, P);
      }
      else
      {
        ivec("ppars", e, 0, b->p_pars_l, P * ns); ivec("ppars", e, 1, b->p_pars_r, P * ns);
      }
    }
    for (int e = 0; e < E && !timing; ++e)
    {
      const int c = Pars(tree->a_edges[e], tree);
      ivec("cpars", e, gp, &c, 1);
      ivec("site", e, gp, tree->site_pars, P);
    }
    if (timing)
    {
      const int R = gp ? (atoi(rep) * 4 / (ns * ns) > 0 ? atoi(rep) * 4 / (ns * ns) : 1) : atoi(rep); /* (the step-matrix loop costs ns * ns per state) */
      Pars(NULL, tree);
      const double t0 = now();
      for (int r = 0; r < R; ++r) Pars(NULL, tree);
      const double dt = now() - t0;
      printf("time_%d_0 ns_per_pattern_update %.4f seconds_per_call %.6e\n", gp, dt * 1e9 / ((double)R * (3.0 * (n - 2) + 1.0) * P), dt / R);
    }
  }
  printf("PARS_END\n");
  return 0;
}
