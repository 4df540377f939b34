// split_run.hip — host side of the object split (include/chanvese_hip.h, "Object split"): the cleaned mask of n contexts taken apart into
// one object per eroded core -- erode, label, grow back, cut -- as int32 labels and a table for the caller, or baked into the members'
// level sets.  Each call is ONE MemberCall (cvh_host.h, io_run.hip) with further waits: the mask source's launches (MaskSource,
// components_run.hip), the erosion pass of morph_kernels.hip and the labelling launches of components_kernels.hip through their host
// entry points, and split_kernels.hip's own.  The growth's sweeps are enqueued CVH_SPLIT_GROUP at a time; the host reads the members'
// counters once per group.  The single forms are batches of one member (guarded_one).  cvh_split* only read; a level-set write ends as
// the cvh_init_* calls do (MemberCall::arrived).
#include "cvh_host.h"

namespace {

struct Outputs {
  int32_t *const *d_labels = nullptr;
  cvh_component *table = nullptr;
  int cap = 0;
  int *counts = nullptr;
  bool levelset = false;
  double inside = 0.0, outside = 0.0;
};

constexpr int kSlots = CVH_SPLIT_GROUP + 1;   // a group's counters: what its first sweep reads, then what each sweep adds to

// staging behind the call's two tables (the mask launches' and the erosion's column table):
// [marker table][key table][tile table][emit table][a word per member: K][kSlots counters per member][the members' parameters];
// host only: the landing place of the words and the counters
struct Staged {
  MemberCall call;
  CvhIoMember *marker = nullptr, *key = nullptr, *tile = nullptr, *emit = nullptr;
  unsigned long long *words = nullptr, *d_words = nullptr;
  unsigned *cnt = nullptr, *d_cnt = nullptr;
  CvhMorphPar *par = nullptr;
  size_t words_off = 0, cnt_off = 0, cnt_bytes = 0, back_bytes = 0;
  unsigned tile_grid = 0, emit_grid = 0;

  template <class T> const T *dev(const T *host) const { return (const T *)(call.db + ((const unsigned char *)host - call.hb)); }
  const unsigned long long *landed_words() const { return (const unsigned long long *)(call.hb + call.host_off); }
  const unsigned *landed_cnt() const { return (const unsigned *)(call.hb + call.host_off + (cnt_off - words_off)); }

  int begin(cvh_context *const *ctxs, int n, const char *what)
  {
    const size_t tab_bytes = align_up((size_t)n * sizeof(CvhIoMember), 256), word_bytes = align_up((size_t)n * sizeof(unsigned long long), 256);
    cnt_bytes = (size_t)kSlots * n * sizeof(unsigned);
    back_bytes = word_bytes + align_up(cnt_bytes, 256);
    const int rc = call.begin(ctxs, n, what, 4 * tab_bytes + back_bytes + (size_t)n * sizeof(CvhMorphPar), back_bytes, true);
    if (rc != CVH_OK) return rc;
    unsigned char *const x = call.hb + call.extra_off;
    marker = (CvhIoMember *)x; key = (CvhIoMember *)(x + tab_bytes); tile = (CvhIoMember *)(x + 2 * tab_bytes); emit = (CvhIoMember *)(x + 3 * tab_bytes);
    words_off = call.extra_off + 4 * tab_bytes; cnt_off = words_off + word_bytes;
    words = (unsigned long long *)(call.hb + words_off); d_words = (unsigned long long *)(call.db + words_off);
    cnt = (unsigned *)(call.hb + cnt_off); d_cnt = (unsigned *)(call.db + cnt_off);
    par = (CvhMorphPar *)(call.hb + words_off + back_bytes);
    return CVH_OK;
  }
};

int split(cvh_context *const *ctxs, int n, const MaskSource &src, const uint32_t *r2, const Outputs &out, void *stream, const char *what)
{
  int rc = src.check(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (!r2) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of squared radii is NULL", what);
  if (out.table && out.cap < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: cap must not be negative, got %d", what, out.cap);
  rc = members_distances_fit(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  bool any_labels = false;
  for (int i = 0; out.d_labels && i < n; ++i) {
    if (!out.d_labels[i]) continue;   // (no label plane for this member)
    rc = element_pointer_check(ctxs, n, i, out.d_labels[i], sizeof(int32_t), what);
    if (rc != CVH_OK) return rc;
    any_labels = true;
  }
  rc = src.ready(ctxs, n, what, true);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    rc = ensure_workspace(c, &c->d_morph, cvh_morph_workspace_bytes(c->h, c->w), "morphology", false);
    const bool fresh = rc == CVH_OK && !c->d_split;
    if (rc == CVH_OK) rc = ensure_workspace(c, &c->d_split, cvh_split_workspace_bytes(c->h, c->w), "split", false);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, c->err);
    // the keys past the plane's last row and column are outside F0 for good: no launch writes them
    if (fresh) HIPCHK(lead, hipMemsetAsync(c->d_split, 0, cvh_split_workspace_bytes(c->h, c->w), lead->stream));
  }
  Staged st;
  rc = st.begin(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  MemberCall &call = st.call;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    uint8_t *const base = (uint8_t *)c->d_morph, *const f0 = base + cvh_morph_bytes_offset(c->h, c->w);
    uint8_t *const eroded = base + cvh_score_words_bytes(c->h, c->w), *const dist = base + cvh_morph_dist_offset(c->h, c->w);
    src.fill(&call, i, f0, st.d_words + i, true);   // the mask launches, and the labelling of F0 from its bytes
    CvhIoMember &t = call.tab2[i];   // the erosion's column launches: plane[0] -> plane[1]
    t.src = call.tab[i].src;
    t.src2 = f0;
    t.plane[0] = base; t.plane[1] = eroded; t.plane[2] = dist;
    t.nblk = cvh_reinit_column_blocks(c->h, c->w);
    CvhIoMember &m = st.marker[i];   // the marker launches, and the labelling of M from its bytes (behind the erosion, in its distance field's place)
    m = call.tab[i];
    m.src = f0; m.src2 = eroded; m.dst = dist;
    const int ty = cvh_split_tiles_y(c->h), tx = cvh_split_tiles_x(c->w);
    CvhIoMember &k = st.key[i];
    k = call.tab[i];
    k.src = c->d_cc; k.src2 = f0; k.dst = nullptr; k.sums = nullptr;
    k.plane[0] = (uint8_t *)c->d_split; k.plane[1] = k.plane[2] = nullptr;
    k.w2 = tx * CVH_SPLIT_TILE_COLS;
    CvhIoMember &g = st.tile[i];
    g = k;
    g.src = g.src2 = nullptr;
    g.h2 = ty * CVH_SPLIT_TILE_ROWS; g.interleaved = tx;
    g.sums = (unsigned long long *)(st.d_cnt + i);
    g.nblk = (unsigned)ty * (unsigned)tx;
    CvhIoMember &e = st.emit[i];
    e = k;
    e.src = e.src2 = nullptr;
    if (out.levelset) levelset_target(c, &e);
    else e.dst = out.d_labels ? out.d_labels[i] : nullptr;
    e.nblk = cvh_split_emit_blocks(c->n);
    CvhMorphPar &p = st.par[i];
    p.inside = out.inside; p.outside = out.outside; p.r2 = r2[i]; p.root = disk_root(r2[i]);
    st.cnt[i] = 1;   // slot 0: the first sweep runs
  }
  lay_out(st.marker, n);   // (the sections of the call's first table, which run() lays out)
  lay_out(st.key, n);
  st.tile_grid = lay_out(st.tile, n);
  st.emit_grid = lay_out(st.emit, n);
  static const bool kErode[1] = {true};
  auto sweeps_and_back = [&]() -> int {
    HIPCHK(lead, cvh_launch_split_sweeps(st.dev(st.tile), n, st.tile_grid, src.conn, CVH_SPLIT_GROUP, lead->stream));
    HIPCHK(lead, hipMemcpyAsync(call.hb + call.host_off, call.db + st.words_off, st.back_bytes, hipMemcpyDeviceToHost, lead->stream));
    return CVH_OK;
  };
  // the FIRST wait: the counts and the first group's counters
  rc = call.run(stream, false, true, [&]() -> int {
    const int rc_mask = src.launch(call, true);   // F0 as bytes, raw or cleaned
    if (rc_mask != CVH_OK) return rc_mask;
    HIPCHK(lead, cvh_launch_morph_bits(call.dtab2(), n, call.grid2, false, 0, lead->stream));
    HIPCHK(lead, cvh_launch_morph_passes(call.dtab2(), st.dev(st.par), n, call.grid2, 1, kErode, lead->stream));
    HIPCHK(lead, cvh_launch_cc_number(call.dtab(), n, call.grid, 1, src.conn, 0, lead->stream));   // F0's forest
    HIPCHK(lead, cvh_launch_split_markers(st.dev(st.marker), n, call.grid, lead->stream));
    HIPCHK(lead, cvh_launch_cc_number(st.dev(st.marker), n, call.grid, 1, src.conn, 0, lead->stream));   // M's, numbered: K
    HIPCHK(lead, cvh_launch_split_keys(st.dev(st.key), n, call.grid, lead->stream));
    return sweeps_and_back();
  });
  if (rc != CVH_OK) return rc;
  ++g_launches[kSplitLaunchSets];
  // a group more, and a wait more, until a sweep has changed nothing in any member
  for (;;) {
    const unsigned *got = st.landed_cnt();
    bool done = true;
    unsigned long ran = 0;
    for (int j = 0; j < kSlots; ++j) {
      bool any = false;
      for (int i = 0; i < n; ++i) any = any || got[(size_t)j * n + i] != 0;
      if (j < CVH_SPLIT_GROUP) ran += any ? 1 : 0;
      else done = !any;
    }
    g_launches[kSplitSweeps] += ran;
    if (done) break;
    memset(st.cnt, 0, st.cnt_bytes);
    for (int i = 0; i < n; ++i) st.cnt[i] = got[(size_t)CVH_SPLIT_GROUP * n + i];
    HIPCHK(lead, hipMemcpyAsync(st.d_cnt, st.cnt, st.cnt_bytes, hipMemcpyHostToDevice, lead->stream));
    rc = sweeps_and_back();
    if (rc == CVH_OK) rc = call.wait_again(stream, false);
    if (rc != CVH_OK) return rc;
  }
  const unsigned long long *words = st.landed_words();
  for (int i = 0; out.counts && i < n; ++i) out.counts[i] = (int)words[i];
  const size_t K = (size_t)words[0], rows = std::min<size_t>(K, out.table ? (size_t)out.cap : 0);
  if (!rows && !any_labels && !out.levelset) return CVH_OK;
  // the cut and the outputs, the rows of the single form's table, and the LAST wait
  if (any_labels || out.levelset)
    HIPCHK(lead, cvh_launch_split_emit(st.dev(st.emit), st.dev(st.par), n, st.emit_grid, out.levelset, lead->stream));
  if (rows) {
    rc = grow_table_to(lead, &lead->cc_table, K, K + K / 4, (K + K / 4) * sizeof(cvh_component));
    if (rc != CVH_OK) return rc;
    st.key[0].dst = lead->cc_table.d;
    rc = call.upload_again(st.key);
    if (rc != CVH_OK) return rc;
    HIPCHK(lead, cvh_launch_split_table(st.dev(st.key), 1, st.key[0].nblk, lead->stream));
    HIPCHK(lead, hipMemcpyAsync(out.table, lead->cc_table.d, rows * sizeof(cvh_component), hipMemcpyDeviceToHost, lead->stream));
  }
  rc = call.wait_again(stream, any_labels);
  if (rc != CVH_OK) return rc;
  return out.levelset ? call.arrived() : CVH_OK;
}

}  // namespace

extern "C" void cvh_split_geometry(int *tile_rows, int *tile_cols, int *group)
{
  if (tile_rows) *tile_rows = CVH_SPLIT_TILE_ROWS;
  if (tile_cols) *tile_cols = CVH_SPLIT_TILE_COLS;
  if (group) *group = CVH_SPLIT_GROUP;
}

extern "C" int cvh_split_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                               const uint32_t *r2, int32_t *const *d_labels, int *counts, void *stream)
{
  static const char what[] = "cvh_split_batch";
  return guarded(ctxs, n, what, [&]() {
    Outputs out;
    out.d_labels = d_labels; out.counts = counts;
    return split(ctxs, n, {conn, invert, min_area, fill_holes, keep_largest}, r2, out, stream, what);
  });
}

extern "C" int cvh_split(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, uint32_t r2, int32_t *d_labels,
                         cvh_component *table, int cap, int *count, void *stream)
{
  return guarded_one(c, "cvh_split", [&](const char *what) {
    Outputs out;
    out.d_labels = &d_labels; out.table = table; out.cap = cap; out.counts = count;
    return split(&c, 1, {conn, invert, min_area, fill_holes, keep_largest}, &r2, out, stream, what);
  });
}

// the host form: the labels land in the int32 plane the overlaps' host form stages (4 bytes per pixel, the context's), on the context's
// stream, and come down behind the call's last wait
extern "C" int cvh_split_host(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, uint32_t r2, int32_t *labels,
                              cvh_component *table, int cap, int *count)
{
  return guarded_one(c, "cvh_split_host", [&](const char *what) -> int {
    if (!labels) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: labels is NULL", what);
    const MaskSource src = {conn, invert, min_area, fill_holes, keep_largest};
    int rc = src.check(&c, 1, what);
    if (rc == CVH_OK) rc = members_below(&c, 1, what, 31);
    if (rc == CVH_OK) rc = members_have_levelsets(&c, 1, what);   // before the plane is allocated
    if (rc != CVH_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_workspace(c, &c->d_overlap_plane, c->n * sizeof(int32_t), "label plane", false);
    if (rc != CVH_OK) return batch_fail(&c, 1, rc, "%s: %s", what, std::string(c->err).c_str());
    int32_t *d_labels = (int32_t *)c->d_overlap_plane;
    Outputs out;
    out.d_labels = &d_labels; out.table = table; out.cap = cap; out.counts = count;
    rc = split(&c, 1, src, &r2, out, c->stream, what);
    if (rc != CVH_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(labels, d_labels, c->n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CVH_OK;
  });
}

extern "C" int cvh_split_levelset_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                        const uint32_t *r2, double inside, double outside)
{
  static const char what[] = "cvh_split_levelset_batch";
  return guarded(ctxs, n, what, [&]() {
    Outputs out;
    out.levelset = true; out.inside = inside; out.outside = outside;
    return split(ctxs, n, {conn, invert, min_area, fill_holes, keep_largest}, r2, out, nullptr, what);
  });
}

extern "C" int cvh_split_levelset(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, uint32_t r2,
                                  double inside, double outside)
{
  return guarded_one(c, "cvh_split_levelset", [&](const char *what) {
    Outputs out;
    out.levelset = true; out.inside = inside; out.outside = outside;
    return split(&c, 1, {conn, invert, min_area, fill_holes, keep_largest}, &r2, out, nullptr, what);
  });
}
