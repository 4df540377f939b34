// march_flow.h — the ONE call sequence of the marching-wave flows (four phases, localised regions, edge-weighted length, convex relaxation) over a flow
// description F, which multiphase_run.hip, localized_run.hip, geodesic_run.hip and convex_run.hip each supply and a new march flow has to:
//   types      Args (the record: its fields u, st_mirror, trace, trace_cap by those names), State (begins with CvhMarchCount run), Geom
//   constants  kStateBytes (the workspace's state section), kSlotBytes (a slot of the leader's state table), kPer (contexts per member),
//              kWorkspace (its name in messages), kZeroState (no launch in front of iteration 0 writes the state block: zeroed here)
//   members    all (the call's contexts, flat: [member][role]), rules(n, i, what, who) (member i's refusals: march_rules and the flow's
//              own), geometry(i), workspace_bytes(i, g), args(i, g, rec) (everything of the record but what a run adds)
//   static     workspace(c) (the slot in a member's first context), trace_table(c), row_width(C), blocks(g) (the member's share of the
//              largest launch), sections(rec) (its prefix counts and grids), norms_out(st, i, norms), and per class present
//              before(lead, tab, q, one) (what precedes iteration 0) and step(lead, tab, q, parity, one)
#pragma once
#include "cvh_host.h"

// a record's prefix block count and own workgroups in each of a flow's (one or two) launch grids; first[1] null: one grid
struct MarchSections { unsigned *first[2]; unsigned grid[2]; };

// order[r]: the member record r describes -- members sorted by class, in member order inside a class; cls[k]: class k's section
template <class ClassOf>
void march_classes(int n, ClassOf class_of, std::vector<int> *order, MarchClass *cls)
{
  order->clear();
  for (int k = 0; k < kMarchClasses; ++k) {
    cls[k] = MarchClass{};
    cls[k].first = (int)order->size();
    cls[k].C = k < 2 ? 1 : 3;
    cls[k].fast = k & 1;
    for (int i = 0; i < n; ++i)
      if (class_of(i) == k) order->push_back(i);
    cls[k].n = (int)order->size() - cls[k].first;
  }
}

// the sections of a class's grids: record r owns its member's own grid(s) behind those of the records of its class before it
template <class Args, class Sections>
void march_lay_out(Args *recs, MarchClass *cls, Sections sections)
{
  for (int k = 0; k < kMarchClasses; ++k) {
    unsigned sum[2] = {0, 0};
    for (int r = cls[k].first; r < cls[k].first + cls[k].n; ++r) {
      const MarchSections s = sections(recs[r]);
      for (int j = 0; j < 2 && s.first[j]; ++j) { *s.first[j] = sum[j]; sum[j] += s.grid[j]; }
    }
    cls[k].grid = sum[0]; cls[k].grid2 = sum[1];
  }
}

// body(tab, q) -- the launches over class q's records tab[0 .. q.n - 1] -- for each class present
template <class Args, class Body>
int march_each_class(const Args *d_recs, const MarchClass *cls, Body body)
{
  for (int k = 0; k < kMarchClasses; ++k) {
    if (!cls[k].n) continue;
    const int rc = body(d_recs + cls[k].first, cls[k]);
    if (rc != CVH_OK) return rc;
  }
  return CVH_OK;
}

// every member's refusals, and the batch's: a launch over all members stays below 2^31 workgroups
template <class F>
int march_batch_rules(const F &f, int n, const char *what)
{
  unsigned long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    const int rc = f.rules(n, i, what, member_prefix(i).c_str());
    if (rc != CVH_OK) return rc;
    blocks += F::blocks(f.geometry(i));
    if (blocks >= (1ull << 31))
      return batch_fail(f.all, n * F::kPer, CVH_ERR_ARG, "%s: member %d: the members up to this one need 2^31 workgroups or more in one launch", what, i);
  }
  return CVH_OK;
}

// the contexts of n members settled, their FP64 mirrors fresh, every member's workspace there
template <class F>
int march_ready(const F &f, int n, const char *what, const typename F::Geom *g)
{
  cvh_context *const *all = f.all;
  HIPCHK(all[0], hipSetDevice(all[0]->device));
  int rc = settle_all(all, n * F::kPer, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(all, n * F::kPer, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = all[(size_t)i * F::kPer];
    void **slot = F::workspace(c);
    const bool fresh = !*slot;
    rc = ensure_workspace(c, slot, f.workspace_bytes(i, g[i]), F::kWorkspace, false);
    if (rc != CVH_OK) return batch_fail(all, n * F::kPer, rc, "%s: %s", what, c->err);
    if (F::kZeroState && fresh) HIPCHK(c, hipMemsetAsync(*slot, 0, F::kStateBytes, c->stream));   // a state block never holds what hipMalloc left there
  }
  return CVH_OK;
}

// recs[0 .. n-1]: the members' records in class order -- but the state slot and the trace, which a run adds -- and the classes laid out
template <class F>
void march_records(const F &f, int n, const typename F::Geom *g, typename F::Args *recs, std::vector<int> *order, MarchClass *cls)
{
  march_classes(n, [&](int i) { return march_class(f.all[(size_t)i * F::kPer]); }, order, cls);
  for (int r = 0; r < n; ++r) f.args((*order)[r], g[(*order)[r]], &recs[r]);
  march_lay_out(recs, cls, F::sections);
}

// a call that launches for ONE checked member by value and does not iterate (the means calls): the member ready, its record, its class
template <class F>
int march_single(const F &f, const char *what, typename F::Args *m, MarchClass *cls)
{
  const typename F::Geom g = f.geometry(0);
  const int rc = march_ready(f, 1, what, &g);
  if (rc != CVH_OK) return rc;
  std::vector<int> order;
  march_records(f, 1, &g, m, &order, cls);
  return CVH_OK;
}

// A run of n checked members (MarchRun, cvh_host.h); who(k) opens what a message says about context f.all[k].  steps_done[n], norms
// (as F::norms_out lays them out), traces[n] / rows[n] may be null.  bake(k, done), if given, brings context k's level set into the buffer a new
// one lands in itself (MarchRun::bake): a flow whose iterated planes are not the level set
template <class F>
int march_run(const F &f, int n, int max_steps, int *steps_done, double *norms, double *const *traces, int trace_rows, int *rows, const char *what,
              const std::function<std::string(int)> &who, const std::function<int(int, int)> &bake = nullptr)
{
  using Args = typename F::Args;
  cvh_context *const *all = f.all;
  cvh_context *lead = all[0];
  auto first_of = [&](int i) { return all[(size_t)i * F::kPer]; };
  MarchRun run{all, n, F::kPer, what, who};
  run.bake = bake;
  int rc = run.begin(max_steps, traces, trace_rows, rows);
  if (rc != CVH_OK) return rc;
  std::vector<typename F::Geom> g((size_t)n);
  for (int i = 0; i < n; ++i) g[i] = f.geometry(i);
  rc = march_ready(f, n, what, g.data());
  if (rc != CVH_OK) return rc;
  for (int k = 0; k < n * F::kPer; ++k) {   // the stop norms and the plane sums (taken again where the planes changed on the device)
    rc = prepare_host(all[k]);
    if (rc != CVH_OK) return batch_fail(all, n * F::kPer, rc, "%s: %s%s", what, who(k).c_str(), all[k]->err);
  }
  rc = run.open([&](int i) { return F::trace_table(first_of(i)); }, [&](int i) { return F::row_width(first_of(i)->C); }, sizeof(Args), F::kSlotBytes);
  if (rc != CVH_OK) return rc;
  std::vector<int> order;
  MarchClass cls[kMarchClasses];
  Args *recs = (Args *)run.record(0);
  march_records(f, n, g.data(), recs, &order, cls);
  for (int r = 0; r < n; ++r) {
    const int i = order[r];
    recs[r].st_mirror = (typename F::State *)run.d_state(i);
    recs[r].trace = run.d_trace[i]; recs[r].trace_cap = run.trace_cap[i];
    if (F::kZeroState) HIPCHK(lead, hipMemsetAsync(*F::workspace(first_of(i)), 0, F::kStateBytes, lead->stream));
  }
  // ONE member: its record travels by value -- u[0] read, u[1] written, swapped here per iteration -- nothing is uploaded, and the host
  // reads the member's own state block: the single call's launches as they were before the batch existed
  Args *one = n == 1 ? recs : nullptr;
  decltype(recs->u) bufs;   // [parity]: the member's buffer(s) as the record was filled
  memcpy(bufs, recs->u, sizeof(bufs));
  if (one) run.own_state = *F::workspace(lead);
  else rc = run.upload();
  if (rc != CVH_OK) return rc;
  const Args *d_recs = (const Args *)run.d_record(0);
  rc = march_each_class(d_recs, cls, [&](const Args *tab, const MarchClass &q) { return F::before(lead, tab, q, one); });
  if (rc != CVH_OK) return rc;
  rc = run.iterate([&](int parity) {
    if (one) { memcpy(&one->u[0], &bufs[parity], sizeof(bufs[0])); memcpy(&one->u[1], &bufs[parity ^ 1], sizeof(bufs[0])); }
    return march_each_class(d_recs, cls, [&](const Args *tab, const MarchClass &q) { return F::step(lead, tab, q, parity, one); });
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const typename F::State *st = (const typename F::State *)run.state(i);
    if (steps_done) steps_done[i] = st->run.steps_done;
    if (norms) F::norms_out(*st, i, norms);
  }
  return CVH_OK;
}
