// csv_batch.hip — the fused batch: N contexts advance together, one launch per iteration and CSV-step instantiation (cvh_enqueue_steps_batch,
// cvh_run_batch); and what every batch of contexts shares (member and pair checks, member predicates -- shapes, state, the capacities of
// output arrays --, errors, stream joins, the grow-only device buffers: grow_table by bytes, grow_table_to by elements).
#include "cvh_host.h"

// The grid of a group is the concatenation of its members' own grids (nparts workgroups + the chain-mode bookkeeper), each padded to a
// multiple of 8 workgroups (CvhBatchArgs, cvh_internal.h).  A member's launch arguments differ between its iterations only with period 4
// (ping-pong parity x chain-mode sum set, see ensure_step_graph): the four phases of every member are uploaded once, when the batch's
// composition or a member's arguments change, and an iteration's launch passes two pointers.
struct BatchGroup {
  CvhStepArgs rep;          // the first member's arguments: select the instantiation (every member of the group has the same)
  int kind = 0, C = 1, fast = 0;
  int n = 0;                // members
  unsigned grid = 0;        // workgroups, padding included
  size_t args_off = 0, map_off = 0;   // byte offsets in BatchCache::table: [4][n] CvhStepArgs, grid / 8 CvhBatchEntry
};
struct BatchCache {
  std::vector<cvh_context *> members;
  std::vector<unsigned char> image;   // what table holds
  std::vector<BatchGroup> groups;
  DeviceTable table;                  // d's bytes on the device
  int rot = 0;                        // phase of the tables an enqueue starts at
};

// t holds at least `bytes` bytes afterwards (what it held is lost when it grows)
int grow_table(cvh_context *c, DeviceTable *t, size_t bytes)
{
  if (t->cap >= bytes) return CVH_OK;
  free_table(t);
  HIPCHK(c, hipMalloc(&t->d, bytes));
  t->cap = bytes;
  return CVH_OK;
}

// t holds at least `want` elements afterwards: where it has fewer it is allocated anew, `count` elements in `bytes` bytes -- the rule
// that sizes both is the caller's (what it held is lost when it grows)
int grow_table_to(cvh_context *c, DeviceTable *t, size_t want, size_t count, size_t bytes)
{
  if (t->count >= want) return CVH_OK;
  free_table(t);
  HIPCHK(c, hipMalloc(&t->d, bytes));
  t->cap = bytes; t->count = count;
  return CVH_OK;
}

void free_table(DeviceTable *t)
{
  if (t->d) (void)hipFree(t->d);
  t->d = nullptr; t->cap = t->count = 0;
}

void batch_cache_free(cvh_context *c)
{
  if (!c->batch) return;
  free_table(&c->batch->table);
  delete c->batch;
  c->batch = nullptr;
}

// batch errors: the message goes to member 0 (if there is one) and to cvh_last_error(NULL)
int batch_fail(cvh_context *const *ctxs, int n, int code, const char *fmt, ...)
{
  char msg[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
  snprintf(create_err(), kErrLen, "%s", msg);
  if (ctxs && n >= 1 && ctxs[0]) snprintf(ctxs[0]->err, sizeof(ctxs[0]->err), "%s", msg);
  return code;
}

// Who may be in a batch: what can be refused before anything is touched (the members stay as they were).  `what` opens the message
// ("batch", or the entry point's name); `needs` says how much a member must hold -- the list alone (device-memory I/O), an image
// (a Perona-Malik batch needs no level set and no CSV geometry), or all a fused CSV launch takes (the two batches': their texts say "batch").
int members_check(cvh_context *const *ctxs, int n, const char *what, MemberNeeds needs)
{
  if (!ctxs || n < 1) return batch_fail(ctxs, 0, CVH_ERR_ARG, "%s: empty member list (ctxs = %p, n = %d)", what, (const void *)ctxs, n);
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    if (!c) return batch_fail(ctxs, i ? n : 0, CVH_ERR_ARG, "%s: member %d is NULL", what, i);
    for (int j = 0; j < i; ++j)
      if (ctxs[j] == c) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d duplicates member %d", what, i, j);
    if (c->device != ctxs[0]->device)
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d is on device %d, member 0 on device %d", what, i, c->device, ctxs[0]->device);
    if (needs == kMembersListed) continue;
    if (!c->have_image) return batch_fail(ctxs, n, CVH_ERR_STATE, "batch: member %d has no image (call cvh_set_image first)", i);
    if (needs == kMembersWithImage) continue;
    if (!c->have_u) return batch_fail(ctxs, n, CVH_ERR_STATE, "batch: member %d has no level set (call cvh_set_levelset or cvh_init_checkerboard first)", i);
    if (c->finalize_mode != 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "batch: member %d has finalize = 1 (a separate finalise kernel per launch): no fused batch", i);
    const Geometry g = resolve_geometry(c);
    if (g.strip < 2) return batch_fail(ctxs, n, CVH_ERR_ARG, "batch: member %d (%d x %d) takes the tile kernel: no fused batch", i, c->h, c->w);
  }
  return CVH_OK;
}

// Member predicates: what a call refuses for its members' shapes and state before anything is touched.  Each goes through members
// 0 .. n-1 in order -- or, with only >= 0, looks at that member alone: for a caller that interleaves it with a rule of its own.

// planes of fewer than 2^k pixels: what the indices of the call's kernels cover
int members_below(cvh_context *const *ctxs, int n, const char *what, int k, int only)
{
  for (int i = std::max(only, 0); i < (only < 0 ? n : only + 1); ++i)
    if (ctxs[i]->n >= ((size_t)1 << k))
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %d x %d is too large, h * w must stay below 2^%d", what, i, ctxs[i]->h, ctxs[i]->w, k);
  return CVH_OK;
}

// squared distances are 32-bit integers, vertical distances 16-bit with one value set aside: cvh_reinit's passes and the calls that share them
int members_distances_fit(cvh_context *const *ctxs, int n, const char *what, int only)
{
  for (int i = std::max(only, 0); i < (only < 0 ? n : only + 1); ++i) {
    const cvh_context *c = ctxs[i];
    if ((unsigned long long)c->h * c->h + (unsigned long long)c->w * c->w >= (1ull << 32))
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %d x %d is too large, h^2 + w^2 must stay below 2^32", what, i, c->h, c->w);
  }
  return CVH_OK;
}

// the capacities of the members' output arrays: where lists[i] is given (lists may be null, and so may an entry) there are caps --
// `without` is the refusal otherwise -- and caps[i], which the refusal calls `noun`, is not negative
template <class T>
int members_caps_fit(cvh_context *const *ctxs, int n, const char *what, const void *const *lists, const T *caps, const char *noun, const char *without,
                     int only)
{
  for (int i = std::max(only, 0); lists && i < (only < 0 ? n : only + 1); ++i) {
    if (!lists[i]) continue;
    if (!caps) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: %s", what, without);
    if (caps[i] < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %s must not be negative, got %ld", what, i, noun, (long)caps[i]);
  }
  return CVH_OK;
}
template int members_caps_fit<int>(cvh_context *const *, int, const char *, const void *const *, const int *, const char *, const char *, int);
template int members_caps_fit<long>(cvh_context *const *, int, const char *, const void *const *, const long *, const char *, const char *, int);

int members_have_images(cvh_context *const *ctxs, int n, const char *what)
{
  for (int i = 0; i < n; ++i)
    if (!ctxs[i]->have_image) return batch_fail(ctxs, n, CVH_ERR_STATE, "%s: member %d has no image (call cvh_set_image first)", what, i);
  return CVH_OK;
}

int members_have_levelsets(cvh_context *const *ctxs, int n, const char *what, int only)
{
  for (int i = std::max(only, 0); i < (only < 0 ? n : only + 1); ++i)
    if (!ctxs[i]->have_u) return batch_fail(ctxs, n, CVH_ERR_STATE, "%s: member %d has no level set", what, i);
  return CVH_OK;
}

// the FP64 mirrors of members first .. n-1 hold their level sets (ensure_f64_mirror); a failure names `noun` i - first
int members_mirrors_fresh(cvh_context *const *ctxs, int n, const char *what, int first, const char *noun)
{
  for (int i = first; i < n; ++i) {
    const int rc = ensure_f64_mirror(ctxs[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: %s %d: %s", what, noun, i - first, ctxs[i]->err);
  }
  return CVH_OK;
}

// Who may be in a call on n pairs of contexts: what can be refused before anything is touched.  *all = [dst 0 .. n-1, src 0 .. n-1],
// the call's member list, is filled here.  The lists themselves, then args() (the call's other arguments, if any), then pair by pair:
// the device, rule(i) -- the call's shape and channel rule, which returns CVH_OK or has called batch_fail on *all --, and the size of
// the pair's larger context, the first list's (row and column indices and a lane's item index stay 32-bit).
int pairs_check(const PairRoles &p, int n, const char *what, std::vector<cvh_context *> *all, const std::function<int(int)> &rule,
                const std::function<int()> &args)
{
  if (!p.first || !p.second || n < 1)
    return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: empty pair list (%s = %p, %s = %p, n = %d)", what, p.first_name, (const void *)p.first, p.second_name,
                      (const void *)p.second, n);
  for (int i = 0; i < n; ++i)
    if (!p.first[i] || !p.second[i])
      return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: pair %d: the %s context is NULL", what, i, p.first[i] ? p.second_role : p.first_role);
  cvh_context *const *dst = p.second_is_dst ? p.second : p.first, *const *src = p.second_is_dst ? p.first : p.second;
  all->assign(dst, dst + n);
  all->insert(all->end(), src, src + n);
  cvh_context *const *ctxs = all->data();
  auto role = [&](int i) { return (i < n) == p.second_is_dst ? p.second_role : p.first_role; };
  for (int i = 0; i < 2 * n; ++i)
    for (int j = 0; j < i; ++j)
      if (ctxs[i] == ctxs[j])
        return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: its %s context is also pair %d's %s context (a context may be listed once)", what, i % n,
                          role(i), j % n, role(j));
  if (args) { const int rc = args(); if (rc != CVH_OK) return rc; }
  for (int i = 0; i < n; ++i) {
    const cvh_context *a = p.first[i], *b = p.second[i];
    for (const cvh_context *x : {a, b})
      if (x->device != ctxs[0]->device)
        return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: its %s context is on device %d, pair 0's on device %d", what, i,
                          x == a ? p.first_role : p.second_role, x->device, ctxs[0]->device);
    const int rc = rule(i);
    if (rc != CVH_OK) return rc;
    if (a->n >= ((size_t)1 << 32))
      return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: %d x %d is too large, h * w must stay below 2^32", what, i, a->h, a->w);
  }
  return CVH_OK;
}

// the sources of a pairs_check'ed call, members n .. 2n-1 of its list, hold images
int pair_sources_have_images(cvh_context *const *all, int n, const char *what, const char *role)
{
  for (int i = 0; i < n; ++i)
    if (!all[n + i]->have_image)
      return batch_fail(all, 2 * n, CVH_ERR_STATE, "%s: pair %d: the %s context has no image (call cvh_set_image first)", what, i, role);
  return CVH_OK;
}

// Automatic geometry of a member: its strips are sized for its share of the chip, num_cus x n_i / sum n (an explicit strip_rows / strips wins)
// -- where its own full-chip strips are short.  The share exists to lengthen strips that the whole-chip grid makes short (every strip re-reads
// 3 halo rows and fills its pipeline once): 8 x 1024^2 4.9 against 6.7 us per image-iteration with the full-chip strips of 8 rows.  Where the
// member's own strips already have kBatchOwnRows rows or more, the share only coarsens its grid into one round of long strips whose
// workgroup count does not divide the CUs (8 x 4096^2: 680 workgroups of 410-row strips, CUs with 2 and with 3 of them, the 2-workgroup
// CUs idle for the last third of the launch -- profiles/r05_fused_batch/timeline_*): such a member keeps its own geometry.
constexpr int kBatchOwnRows = 32;
static void batch_share(cvh_context *const *ctxs, int n, bool on)
{
  double tot = 0.0;
  for (int i = 0; i < n; ++i) tot += (double)ctxs[i]->n;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    c->geom_cus = 0;
    c->in_batch = on;
    if (!on || resolve_geometry(c).strip_rows >= kBatchOwnRows) continue;
    const int share = (int)((double)c->num_cus * (double)c->n / tot + 0.5);
    c->geom_cus = share < 1 ? 1 : share;
  }
}

// Per enqueue: host work of every member (stop condition, strip table), its pending iteration booked if the batch's grid differs from
// the one that left it, its initial sums; then the tables (uploaded only when they changed).  geom_cus is set by the caller.
static int batch_prepare(cvh_context *const *ctxs, int n)
{
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    HIPCHK(c, hipSetDevice(c->device));
    int rc = prepare_host(c);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "batch: member %d: %s", i, c->err);
    const Geometry g = resolve_geometry(c);
    rc = upload_strip_bounds(c, g);
    if (rc == CVH_OK) rc = one_buffer_leave(c);   // a fused batch iterates the pair
    if (rc == CVH_OK) rc = flush_for_grid(c, g.nblocks);
    if (rc == CVH_OK) rc = prepare(c);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "batch: member %d: %s", i, c->err);
  }
  cvh_context *lead = ctxs[0];
  // group the members by CSV-step instantiation (the name cvh_launch_info reports) and dynamic LDS
  std::vector<BatchGroup> groups;
  std::vector<std::string> names;
  std::vector<int> member_group((size_t)n), local((size_t)n);
  std::vector<unsigned> blocks((size_t)n);
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    CvhLaunchNote note{};
    const int rc = launch_one_step(c, (c->cur_base + c->enqueued) & 1, c->enqueued, false, &note);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "batch: member %d: %s", i, c->err);
    char key[160];
    snprintf(key, sizeof(key), "%s lds=%u", note.name, note.lds);
    int gi = 0;
    while (gi < (int)names.size() && names[gi] != key) ++gi;
    if (gi == (int)names.size()) {
      names.push_back(key);
      BatchGroup bg;
      fill_args(c, &bg.rep, (c->cur_base + c->enqueued) & 1, c->enqueued);
      bg.kind = resolve_geometry(c).strip; bg.C = c->C; bg.fast = use_fast(c) ? 1 : 0;
      groups.push_back(bg);
    }
    member_group[i] = gi;
    local[i] = groups[gi].n++;
    blocks[i] = note.grid;
  }
  // the image: per group [4][n] arguments, then the workgroup map
  std::vector<unsigned char> img;
  auto align = [&]() { img.resize((img.size() + 255) & ~(size_t)255); };
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    BatchGroup &bg = groups[gi];
    align();
    bg.args_off = img.size();
    img.resize(img.size() + (size_t)4 * bg.n * sizeof(CvhStepArgs));
    for (int i = 0; i < n; ++i) {
      if (member_group[i] != (int)gi) continue;
      cvh_context *c = ctxs[i];
      for (int q = 0; q < 4; ++q) {
        CvhStepArgs a;
        fill_args(c, &a, (c->cur_base + c->enqueued + q) & 1, c->enqueued + q);
        memcpy(img.data() + bg.args_off + ((size_t)q * bg.n + local[i]) * sizeof(CvhStepArgs), &a, sizeof(a));
      }
    }
    align();
    bg.map_off = img.size();
    unsigned first = 0;
    for (int i = 0; i < n; ++i) {
      if (member_group[i] != (int)gi) continue;
      const unsigned len = (blocks[i] + 7) & ~7u;
      for (unsigned j = 0; j < len; j += 8) {
        const CvhBatchEntry e = {(unsigned)local[i], first, blocks[i], 0u};
        img.insert(img.end(), (const unsigned char *)&e, (const unsigned char *)&e + sizeof(e));
      }
      first += len;
    }
    bg.grid = first;
  }
  // the tables of an enqueue that starts r phases later are the cached ones rotated by r (members advance together)
  BatchCache *bc = lead->batch;
  bool same_members = bc && bc->members.size() == (size_t)n && !memcmp(bc->members.data(), ctxs, (size_t)n * sizeof(cvh_context *));
  if (same_members && bc->image.size() == img.size() && bc->groups.size() == groups.size()) {
    for (int r = 0; r < 4; ++r) {
      bool eq = true;
      for (size_t gi = 0; gi < groups.size() && eq; ++gi) {
        const BatchGroup &bg = groups[gi], &old = bc->groups[gi];
        eq = bg.args_off == old.args_off && bg.map_off == old.map_off && bg.n == old.n && bg.grid == old.grid;
        const size_t row = (size_t)bg.n * sizeof(CvhStepArgs);
        for (int q = 0; q < 4 && eq; ++q)
          eq = !memcmp(img.data() + bg.args_off + (size_t)q * row, bc->image.data() + old.args_off + (size_t)((q + r) & 3) * row, row);
        if (eq) eq = !memcmp(img.data() + bg.map_off, bc->image.data() + old.map_off, (size_t)bg.grid / 8 * sizeof(CvhBatchEntry));
      }
      if (eq) { bc->rot = r; return CVH_OK; }
    }
  }
  if (!bc) { bc = lead->batch = new (std::nothrow) BatchCache(); if (!bc) return batch_fail(ctxs, n, CVH_ERR_NOMEM, "batch: out of host memory"); }
  HIPCHK(lead, hipStreamSynchronize(lead->stream));   // launches already enqueued read the old tables
  const int rc = grow_table(lead, &bc->table, img.size());
  if (rc != CVH_OK) return rc;
  HIPCHK(lead, hipMemcpy(bc->table.d, img.data(), img.size(), hipMemcpyHostToDevice));
  bc->members.assign(ctxs, ctxs + n);
  bc->image.swap(img);
  bc->groups = groups;
  bc->rot = 0;
  return CVH_OK;
}

// The leader's stream (ctxs[0]) waits for what every other member (member[i] != 0, if given) has enqueued on its own.
int join_into_leader(cvh_context *const *ctxs, int n, const int *member)
{
  cvh_context *lead = ctxs[0];
  for (int i = 1; i < n; ++i) {
    if (member && !member[i]) continue;
    HIPCHK(ctxs[i], hipEventRecord(ctxs[i]->ev_join, ctxs[i]->stream));
    HIPCHK(lead, hipStreamWaitEvent(lead->stream, ctxs[i]->ev_join, 0));
  }
  return CVH_OK;
}

// nsteps fused iterations on the leader's stream (joined with every member's stream before, and they with it after)
static int batch_launch(cvh_context *const *ctxs, int n, int nsteps)
{
  cvh_context *lead = ctxs[0];
  BatchCache *bc = lead->batch;
  { const int rc = join_into_leader(ctxs, n); if (rc != CVH_OK) return rc; }
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    if (!c->timing_open) { HIPCHK(c, hipEventRecord(c->ev0, lead->stream)); c->timing_open = true; }
  }
  const unsigned char *d = (const unsigned char *)bc->table.d;
  for (int t = 0; t < nsteps; ++t) {
    const int q = (t + bc->rot) & 3;
    for (const BatchGroup &bg : bc->groups) {
      CvhBatchLaunch bl;
      bl.k.map = (const CvhBatchEntry *)(d + bg.map_off);
      bl.k.args = (const CvhStepArgs *)(d + bg.args_off) + (size_t)q * bg.n;
      bl.grid = bg.grid;
      if (bg.kind == 3) HIPCHK(lead, cvh_launch_wave2(bg.rep, bg.C, bg.fast, lead->stream, &bl));
      else HIPCHK(lead, cvh_launch_wave(bg.rep, bg.C, bg.fast, lead->stream, &bl));
    }
  }
  bc->rot = (bc->rot + nsteps) & 3;
  HIPCHK(lead, hipEventRecord(lead->ev_join, lead->stream));
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    if (i) HIPCHK(c, hipStreamWaitEvent(c->stream, lead->ev_join, 0));
    if (nsteps > 0) {
      const Geometry g = resolve_geometry(c);
      steps_enqueued(c, nsteps, g.nblocks, use_chain(c, g), false);
    }
  }
  return CVH_OK;
}

extern "C" int cvh_enqueue_steps_batch(cvh_context *const *ctxs, int n, int nsteps)
{
  int rc = members_check(ctxs, n, "batch", kMembersForCsv);
  if (rc != CVH_OK) return rc;
  if (nsteps < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "batch: nsteps = %d", nsteps);
  HIPCHK(ctxs[0], hipSetDevice(ctxs[0]->device));
  batch_share(ctxs, n, true);
  for (int i = 0; i < n; ++i) if (nsteps > 0) ctxs[i]->run_chunk = nsteps;
  rc = batch_prepare(ctxs, n);
  if (rc == CVH_OK) rc = batch_launch(ctxs, n, nsteps);
  batch_share(ctxs, n, false);
  return rc;
}

extern "C" int cvh_run_batch(cvh_context *const *ctxs, int n, int max_steps, int *steps_done, double *last_norm)
{
  int rc = members_check(ctxs, n, "batch", kMembersForCsv);
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) {   // every member starts a new run (settles whatever it has in flight first)
    rc = reset_run_impl(ctxs[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "batch: member %d: %s", i, ctxs[i]->err);
  }
  long remaining = max_steps < 0 ? (long)INT_MAX : (long)max_steps;   // src/main.cpp:890, per member
  int chunk_len = INT_MAX;   // the members' pinned status words are polled every sync_every iterations (the smallest of them)
  for (int i = 0; i < n; ++i) if (ctxs[i]->sync_every < chunk_len) chunk_len = ctxs[i]->sync_every;
  if (chunk_len < 1) chunk_len = 1;
  batch_share(ctxs, n, true);
  for (int i = 0; i < n; ++i) ctxs[i]->run_chunk = chunk_len;
  rc = batch_prepare(ctxs, n);
  if (rc == CVH_OK) rc = batch_launch(ctxs, n, 0);   // opens every member's timed interval on the leader's stream
  // Chunks as in cvh_run: launches queued behind a member's stop are no-ops for it (sticky flag); the run ends when every member has
  // stopped or max_steps is reached, never more than kAhead chunks in front of the slowest live member.
  constexpr int kAhead = 4;
  long queued = 0;
  while (rc == CVH_OK && remaining > 0) {
    bool all_stopped = true;
    for (;;) {
      long lag = 0;
      all_stopped = true;
      for (int i = 0; i < n; ++i) {
        volatile int *hs = ctxs[i]->h_status;
        if (hs[1]) continue;
        all_stopped = false;
        if (queued - hs[0] > lag) lag = queued - hs[0];
      }
      if (all_stopped || lag <= (long)kAhead * chunk_len) break;
      if (hipStreamQuery(lead->stream) == hipSuccess) break;   // everything queued has run
    }
    if (all_stopped) break;
    const int chunk = (int)(remaining < chunk_len ? remaining : chunk_len);
    rc = batch_launch(ctxs, n, chunk);
    remaining -= chunk;
    queued += chunk;
  }
  batch_share(ctxs, n, false);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {   // each member's pending iteration is booked (flush) and its run read back
    cvh_context *c = ctxs[i];
    c->timing_open = true;   // sync_impl closes the interval opened on the leader's stream before the first fused launch
    rc = sync_impl(c);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "batch: member %d: %s", i, c->err);
    if (steps_done) steps_done[i] = c->h_state[0].steps_done;
    if (last_norm) last_norm[i] = c->h_state[0].norm;
  }
  return CVH_OK;
}

