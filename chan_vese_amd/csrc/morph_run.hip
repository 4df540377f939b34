// morph_run.hip — host side of the mask morphology and the mask starts (include/chanvese_hip.h, "Mask morphology"): the cleaned mask of n
// contexts dilated, eroded, opened or closed by a disk, as 0/1 bytes for the caller or baked into the members' level sets, and byte masks
// the caller holds as level sets.  Each call is ONE MemberCall (cvh_host.h, io_run.hip: member tables, stream joins, event ordering against
// the caller's stream) around morph_kernels.hip's launches and, where the call cleans, the mask source's (MaskSource, components_run.hip); the single forms
// are batches of one member (guarded_one), and the host forms move their bytes on the context's stream and are then the device forms on
// that stream.  The byte-mask calls only read; a level-set write ends as the cvh_init_* calls do (MemberCall::arrived).
#include "cvh_host.h"

namespace {

struct Levelset { bool write; double inside, outside; };

// staging: [the mask launches' table][the column table][the emit table][one word per member for the cleaning][the members' parameters]
struct Staged {
  MemberCall call;
  CvhIoMember *emit = nullptr;
  const CvhIoMember *d_emit = nullptr;
  CvhMorphPar *par = nullptr;
  const CvhMorphPar *d_par = nullptr;
  unsigned long long *d_words = nullptr;
  unsigned emit_grid = 0;

  int begin(cvh_context *const *ctxs, int n, const char *what)
  {
    const size_t tab_bytes = align_up((size_t)n * sizeof(CvhIoMember), 256), word_bytes = align_up((size_t)n * sizeof(unsigned long long), 256);
    const int rc = call.begin(ctxs, n, what, tab_bytes + word_bytes + (size_t)n * sizeof(CvhMorphPar), 0, true);
    if (rc != CVH_OK) return rc;
    const size_t off = call.extra_off;
    emit = (CvhIoMember *)(call.hb + off); d_emit = (const CvhIoMember *)(call.db + off);
    d_words = (unsigned long long *)(call.db + off + tab_bytes);
    par = (CvhMorphPar *)(call.hb + off + tab_bytes + word_bytes); d_par = (const CvhMorphPar *)(call.db + off + tab_bytes + word_bytes);
    for (int i = 0; i < n; ++i) {
      emit[i] = call.tab[i];   // (n, h, w, C)
      emit[i].nblk = cvh_io_blocks(ctxs[i]->n);
    }
    emit_grid = lay_out(emit, n);
    return CVH_OK;
  }
};

int morph(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, const MaskSource &src, int op, const uint32_t *r2, const Levelset &ls,
          void *stream, const char *what)
{
  int rc = src.check(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (op < CVH_MORPH_NONE || op > CVH_MORPH_CLOSE)
    return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: op must be CVH_MORPH_NONE (0) .. CVH_MORPH_CLOSE (4), got %d", what, op);
  if (!r2) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of squared radii is NULL", what);
  if (!ls.write && !d_masks) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of device pointers is NULL", what);
  rc = members_distances_fit(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; !ls.write && i < n; ++i) { rc = pointer_check(ctxs, n, i, d_masks[i], what); if (rc != CVH_OK) return rc; }
  rc = src.ready(ctxs, n, what, false);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    rc = ensure_workspace(c, &c->d_morph, cvh_morph_workspace_bytes(c->h, c->w), "morphology", false);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, c->err);
  }
  // the passes of the operation: false a dilation, true an erosion (a dilation of the complement within the plane)
  static const bool kPasses[5][2] = {{false, false}, {false, false}, {true, true}, {true, false}, {false, true}};
  const int npass = op == CVH_MORPH_NONE ? 0 : (op == CVH_MORPH_OPEN || op == CVH_MORPH_CLOSE ? 2 : 1);
  Staged st;
  rc = st.begin(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  MemberCall &call = st.call;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    uint8_t *const base = (uint8_t *)c->d_morph, *const bytes = base + cvh_morph_bytes_offset(c->h, c->w);
    src.fill(&call, i, bytes, st.d_words + i, false);   // the mask launches
    CvhIoMember &t = call.tab2[i];   // the column launches
    t.src = call.tab[i].src;
    t.src2 = bytes;
    t.plane[0] = base;
    t.plane[1] = base + cvh_score_words_bytes(c->h, c->w);
    t.plane[2] = base + cvh_morph_dist_offset(c->h, c->w);
    t.nblk = cvh_reinit_column_blocks(c->h, c->w);
    CvhIoMember &e = st.emit[i];
    e.plane[0] = t.plane[npass & 1];
    if (ls.write) levelset_target(c, &e);
    else e.dst = d_masks[i];
    CvhMorphPar &p = st.par[i];
    p.inside = ls.inside; p.outside = ls.outside; p.r2 = r2[i]; p.root = disk_root(r2[i]);
  }
  // a byte mask goes to the caller's stream without a host wait, as cvh_get_mask_clean_device; a level set arrives behind ONE wait, as
  // cvh_init_rect
  rc = call.run(stream, !ls.write, ls.write, [&]() -> int {
    const int rc_mask = src.launch(call, false);   // (of a raw mask nothing: the bits launch reads the level sets)
    if (rc_mask != CVH_OK) return rc_mask;
    HIPCHK(lead, cvh_launch_morph_bits(call.dtab2(), n, call.grid2, !src.cleaned(), src.invert, lead->stream));
    HIPCHK(lead, cvh_launch_morph_passes(call.dtab2(), st.d_par, n, call.grid2, npass, kPasses[op], lead->stream));
    HIPCHK(lead, cvh_launch_morph_emit(st.d_emit, st.d_par, n, st.emit_grid, false, ls.write, lead->stream));
    ++g_launches[kMorphLaunchSets];
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  return ls.write ? call.arrived() : CVH_OK;
}

// u(p) = byte(p) != 0 ? inside : outside for n members: ONE launch, ONE host wait, then every member begins the run its level set opens
int init_mask(cvh_context *const *ctxs, int n, const uint8_t *const *d_masks, double inside, double outside, void *stream, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc == CVH_OK) rc = members_below(ctxs, n, what, 32);
  if (rc != CVH_OK) return rc;
  if (!d_masks) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of device pointers is NULL", what);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) { rc = pointer_check(ctxs, n, i, d_masks[i], what); if (rc != CVH_OK) return rc; }
  rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  Staged st;
  rc = st.begin(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    st.emit[i].src = d_masks[i];
    levelset_target(ctxs[i], &st.emit[i]);
    st.par[i].inside = inside; st.par[i].outside = outside;
    st.call.tab[i].nblk = st.call.tab2[i].nblk = 0;   // (no launch reads these tables)
  }
  rc = st.call.run(stream, false, true, [&]() -> int {
    HIPCHK(lead, cvh_launch_morph_emit(st.d_emit, st.d_par, n, st.emit_grid, true, true, lead->stream));
    ++g_launches[kMorphLaunchSets];
    return CVH_OK;
  });
  return rc != CVH_OK ? rc : st.call.arrived();
}

}  // namespace

extern "C" int cvh_get_mask_morph_device_batch(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int conn, int invert, long min_area,
                                               long fill_holes, int keep_largest, int op, const uint32_t *r2, void *stream)
{
  static const char what[] = "cvh_get_mask_morph_device_batch";
  return guarded(ctxs, n, what, [&]() {
    return morph(ctxs, n, d_masks, {conn, invert, min_area, fill_holes, keep_largest}, op, r2, {false, 0.0, 0.0}, stream, what);
  });
}

extern "C" int cvh_get_mask_morph_device(cvh_context *c, uint8_t *d_mask, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                         int op, uint32_t r2, void *stream)
{
  return guarded_one(c, "cvh_get_mask_morph_device", [&](const char *what) {
    return morph(&c, 1, &d_mask, {conn, invert, min_area, fill_holes, keep_largest}, op, &r2, {false, 0.0, 0.0}, stream, what);
  });
}

extern "C" int cvh_get_mask_morph(cvh_context *c, uint8_t *mask, int conn, int invert, long min_area, long fill_holes, int keep_largest, int op,
                                  uint32_t r2)
{
  return guarded_one(c, "cvh_get_mask_morph", [&](const char *what) {
    if (!mask) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: mask is NULL", what);
    return mask_to_host(c, mask, [&]() {
      return morph(&c, 1, &c->d_mask, {conn, invert, min_area, fill_holes, keep_largest}, op, &r2, {false, 0.0, 0.0}, c->stream, what);
    });
  });
}

extern "C" int cvh_morph_levelset_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                        int op, const uint32_t *r2, double inside, double outside)
{
  static const char what[] = "cvh_morph_levelset_batch";
  return guarded(ctxs, n, what, [&]() {
    return morph(ctxs, n, nullptr, {conn, invert, min_area, fill_holes, keep_largest}, op, r2, {true, inside, outside}, nullptr, what);
  });
}

extern "C" int cvh_morph_levelset(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, int op, uint32_t r2,
                                  double inside, double outside)
{
  return guarded_one(c, "cvh_morph_levelset", [&](const char *what) {
    return morph(&c, 1, nullptr, {conn, invert, min_area, fill_holes, keep_largest}, op, &r2, {true, inside, outside}, nullptr, what);
  });
}

extern "C" int cvh_init_mask_device_batch(cvh_context *const *ctxs, int n, const uint8_t *const *d_masks, double inside, double outside, void *stream)
{
  static const char what[] = "cvh_init_mask_device_batch";
  return guarded(ctxs, n, what, [&]() { return init_mask(ctxs, n, d_masks, inside, outside, stream, what); });
}

extern "C" int cvh_init_mask_device(cvh_context *c, const uint8_t *d_mask, double inside, double outside, void *stream)
{
  return guarded_one(c, "cvh_init_mask_device", [&](const char *what) { return init_mask(&c, 1, &d_mask, inside, outside, stream, what); });
}

extern "C" int cvh_init_mask(cvh_context *c, const uint8_t *mask, double inside, double outside)
{
  return guarded_one(c, "cvh_init_mask", [&](const char *what) {
    if (!mask) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: mask is NULL", what);
    if (c->n >= ((size_t)1 << 32)) return members_below(&c, 1, what, 32);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = settle(c);   // (before the context's stream carries the bytes)
    if (rc != CVH_OK) return rc;
    rc = ensure_workspace(c, &c->d_morph, cvh_morph_workspace_bytes(c->h, c->w), "morphology", false);
    if (rc != CVH_OK) return batch_fail(&c, 1, rc, "%s: %s", what, std::string(c->err).c_str());
    // 1 byte per pixel goes up on the context's stream into the workspace's byte plane, which this call's launch alone reads: the stream
    // orders it behind the copy and, by the call's host wait, in front of the next call's copy
    uint8_t *staged = (uint8_t *)c->d_morph + cvh_morph_bytes_offset(c->h, c->w);
    HIPCHK(c, hipMemcpyAsync(staged, mask, c->n, hipMemcpyHostToDevice, c->stream));
    const uint8_t *d_mask = staged;
    return init_mask(&c, 1, &d_mask, inside, outside, c->stream, what);
  });
}
