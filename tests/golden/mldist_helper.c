/*
 * mldist_helper.c -- TEST INFRASTRUCTURE, compiled by tests/golden/make_mldist.py into a temporary directory against
 * oracle/_ref/libphyml_ref.so (the real reference, built from its sources where they exist).  This repository's own code: it only
 * CALLS the reference's public functions, in the order of its program entry (src/main.c: Get_Input, Get_Seq, Make_Model_Complete,
 * Compact_Data, Init_Model, Set_Model_Parameters -- as oracle/ref_driver.c does), then K80_dist / JC69_Dist as ML_Dist chooses
 * between them (src/lk.c:1812-1814), then ML_Dist, and prints what tests/golden/mldist_<case>.npz holds.  Every double is printed
 * with %a (exact).
 *
 * usage: mldist_helper <phyml command line>
 */
#include <stdio.h>
#include <stdlib.h>

#include "utilities.h"
#include "lk.h"
#include "models.h"
#include "io.h"
#include "init.h"
#include "free.h"

static void vec(const char *name, const double *v, int n)
{
  printf("%s %d", name, n);
  for (int i = 0; i < n; ++i) printf(" %a", v[i]);
  printf("\n");
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

  const int n = cdata->n_otu, P = cdata->n_pattern, S = mod->ns;
  if (io->state_len != 1) return 3;
  matrix *start = (io->datatype == NT && mod->whichmodel < 10) ? K80_dist(cdata, 1E+6) : JC69_Dist(cdata, mod);
  matrix *ml    = ML_Dist(cdata, mod);

  printf("\nMLDIST_BEGIN\n");
  printf("dims 3 %d %d %d\n", n, P, S);
  for (int t = 0; t < n; ++t)
  {
    printf("chars %d ", t);
    for (int p = 0; p < P; ++p) putchar(cdata->c_seq[t]->state[p]);
    printf("\n");
  }
  vec("wght", cdata->wght, P);
  vec("pi", mod->e_frq->pi->v, S);
  vec("e_val", mod->eigen->e_val, S);
  vec("r_e_vect", mod->eigen->r_e_vect, S * S);
  vec("l_e_vect", mod->eigen->l_e_vect, S * S);
  vec("l_min", &mod->l_min, 1);
  vec("l_max", &mod->l_max, 1);
  vec("min_diff_lk_local", &mod->s_opt->min_diff_lk_local, 1);
  for (int j = 0; j < n; ++j)
  {
    char nm[32];
    snprintf(nm, sizeof nm, "start_%d", j);
    vec(nm, start->dist[j], n);
    snprintf(nm, sizeof nm, "dist_%d", j);
    vec(nm, ml->dist[j], n);
  }
  printf("MLDIST_END\n");
  return 0;
}
