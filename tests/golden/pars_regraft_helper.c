/*
 * pars_regraft_helper.c -- TEST INFRASTRUCTURE, compiled by tests/golden/make_pars_regraft.py into a temporary directory against
 * oracle/_ref/libphyml_ref.so (the real reference, built from its sources where they exist).  This repository's own code: it only
 * CALLS the reference's public functions, as pars_helper.c does up to Make_Tree_For_Pars, and then plays the parsimony SPR scan of
 * Test_One_Spr_Target (src/spr.c:639-651) the slow way.  For general_pars = NO and YES and every prune site (edge b, link node -- an
 * internal end of b) named in PARS_REGRAFT_SITES ("all", or "edge:link,edge:link,..."):
 *   Prune_Subtree(link, the other end of b), then for EVERY edge t of the residual tree
 *     Graft_Subtree(t, link, NULL, residual, NULL), Set_Both_Sides(YES), Pars(NULL), Pars(b) -- c_pars and site_pars are printed --
 *     and Prune_Subtree again;
 *   Graft_Subtree onto the edge the first Prune_Subtree named: the tree is whole again, and Pars(NULL) must give what it gave.
 * Every partial vector is made anew by Pars(NULL) on the grafted tree, so nothing here leans on the incremental updates the search
 * itself runs.  Prints what tests/golden/regraft_pars_<case>.npz holds.  Integers only.
 *
 * usage: PARS_REGRAFT_SITES=... [PARS_REGRAFT_KEEP_SITE=1] pars_regraft_helper <phyml command line>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

/* the edges of the subtree behind d, seen from a */
static void mark_subtree(t_node *a, t_node *d, char *in_sub)
{
  if (d->tax) return;
  for (int i = 0; i < 3; ++i)
    if (d->v[i] && d->v[i] != a)
    {
      in_sub[d->b[i]->num] = 1;
      mark_subtree(d, d->v[i], in_sub);
    }
}

int main(int argc, char **argv)
{
  setvbuf(stdout, NULL, _IOLBF, 0); /* (what was printed survives an assertion of the reference) */
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
  const char *spec = getenv("PARS_REGRAFT_SITES");
  const int   keep_site = getenv("PARS_REGRAFT_KEEP_SITE") && atoi(getenv("PARS_REGRAFT_KEEP_SITE")) > 0;
  if (!spec) return 6;

  /* the prune sites: (edge, link) */
  int *site_e = (int *)malloc(sizeof(int) * (size_t)(2 * E)), *site_l = (int *)malloc(sizeof(int) * (size_t)(2 * E)), K = 0;
  if (!strcmp(spec, "all"))
  {
    for (int e = 0; e < E; ++e)
    {
      t_edge *b = tree->a_edges[e];
      if (!b->left->tax) { site_e[K] = e; site_l[K++] = b->left->num; }
      if (!b->rght->tax) { site_e[K] = e; site_l[K++] = b->rght->num; }
    }
  }
  else
  {
    const char *s = spec;
    while (*s && K < 2 * E)
    {
      int e, l, used = 0;
      if (sscanf(s, "%d:%d%n", &e, &l, &used) != 2 || e < 0 || e >= E) return 7;
      site_e[K] = e; site_l[K++] = l;
      s += used;
      if (*s == ',') ++s;
    }
  }

  int  *tmp = (int *)malloc(sizeof(int) * (size_t)(2 * E + 3));
  char *in_sub = (char *)malloc((size_t)E);
  printf("\nPARS_BEGIN\n");
  printf("dims_0_0 4 %d %d %d %d\n", n, P, ns, K);
  for (int e = 0; e < E; ++e) { tmp[2 * e] = tree->a_edges[e]->left->num; tmp[2 * e + 1] = tree->a_edges[e]->rght->num; }
  ivec("edges", 0, 0, tmp, 2 * E);

  for (int gp = 0; gp < 2; ++gp)
  {
    mod->s_opt->general_pars = gp;
    Set_Both_Sides(YES, tree);
    const int whole = Pars(NULL, tree);
    for (int k = 0; k < K; ++k)
    {
      t_edge *b    = tree->a_edges[site_e[k]];
      t_node *link = (b->left->num == site_l[k]) ? b->left : (b->rght->num == site_l[k] ? b->rght : NULL);
      if (!link || link->tax) return 8;
      t_node *d = (link == b->left) ? b->rght : b->left;
      t_edge *target = NULL, *residual = NULL;
      memset(in_sub, 0, (size_t)E);
      mark_subtree(link, d, in_sub);
      Prune_Subtree(link, d, &target, &residual, tree);
      tmp[0] = b->num; tmp[1] = link->num; tmp[2] = d->num;
      if (!gp) ivec("prune", k, 0, tmp, 3);
      int j = 0;
      for (int e = 0; e < E; ++e)
      {
        t_edge *t = tree->a_edges[e];
        if (t == b || t == residual || in_sub[t->num]) continue;
        tmp[0] = t->num; tmp[1] = t->left->num; tmp[2] = t->rght->num;
        if (!gp) ivec("target", k, j, tmp, 3);
        Graft_Subtree(t, link, NULL, residual, NULL, tree);
        Set_Both_Sides(YES, tree);
        Pars(NULL, tree);
        const int c = Pars(b, tree);
        ivec("cp", k * 1000 + j, gp, &c, 1);
        if (keep_site) ivec("sp", k * 1000 + j, gp, tree->site_pars, P);
        t_edge *t2 = NULL, *r2 = NULL;
        Prune_Subtree(link, (link == b->left) ? b->rght : b->left, &t2, &r2, tree);
        if (t2 != t || r2 != residual) return 9; /* (the edge structures keep their roles: src/utilities.c:6210-6223, :6608-6740) */
        ++j;
      }
      tmp[0] = j;
      if (!gp) ivec("ntargets", k, 0, tmp, 1);
      Graft_Subtree(target, link, NULL, residual, NULL, tree);
      Set_Both_Sides(YES, tree);
      if (Pars(NULL, tree) != whole) return 10;
    }
  }
  printf("PARS_END\n");
  return 0;
}
