// io_run.hip — host side of the device-memory entry points (include/chanvese_hip.h): contexts and batches of contexts are fed from, and
// read into, device memory the caller owns, ordered against the caller's stream by events; one launch per batch and operation.
// The single-context calls are batches of one member: one code path.  Reinitialisation (cvh_reinit, cvh_reinit_batch) lives here too: it
// is a level set leaving and arriving without crossing to the host, on the same member tables and stream joins.  MemberCall (cvh_host.h)
// is the scaffold of every member-table call, here and in init_run.hip, components_run.hip, pyramid_run.hip and colour_run.hip: staging,
// the level-set target, the joined launch, the members' arrival, a further host wait (upload_again, wait_again).  write_planes is the one path of the calls that replace planes -- the
// ingest here, the conversions and the luma of colour_run.hip, the local statistics and the rank planes of window_run.hip, the restrict of pyramid_run.hip -- and g_launches the one table of launch
// counters.  What a call refuses for its members or pairs is in csv_batch.hip.  cvh_init_checkerboard is a checkerboard batch of one.
#include <memory>
#include <thread>

#include "cvh_host.h"

std::atomic<unsigned long> g_launches[kLaunchCounters];

// p must be memory that kernels on member i's device can address: device memory of that device, managed memory, or mapped host memory
int pointer_check(cvh_context *const *ctxs, int n, int i, const void *p, const char *what)
{
  if (!p) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: the device pointer is NULL", what, i);
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) (void)hipGetLastError();   // (an address the runtime does not know: not sticky)
  const bool ok = e == hipSuccess && ((at.type == hipMemoryTypeDevice && at.device == ctxs[i]->device) || at.type == hipMemoryTypeManaged ||
                                      (at.type == hipMemoryTypeHost && at.devicePointer != nullptr));
  if (!ok) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %p is not device-accessible memory of device %d", what, i, p, ctxs[i]->device);
  return CVH_OK;
}

// pointer_check for an array of elements of `size` bytes, to which p must be aligned
int element_pointer_check(cvh_context *const *ctxs, int n, int i, const void *p, size_t size, const char *what)
{
  const int rc = pointer_check(ctxs, n, i, p, what);
  if (rc != CVH_OK) return rc;
  if ((uintptr_t)p % size) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %p is not aligned to %zu bytes", what, i, p, size);
  return CVH_OK;
}

// iterations enqueued and never synchronised are closed first, as the host-buffer calls do
int settle_all(cvh_context *const *ctxs, int n, const char *what)
{
  for (int i = 0; i < n; ++i) {
    const int rc = settle(ctxs[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, ctxs[i]->err);
  }
  return CVH_OK;
}

// The leader's staging of a call: `host_bytes` of pinned memory (its first `dev_bytes` are uploaded to the device table).  The pinned
// block is rewritten only when the last copy that read it has completed: the HOST WAITS here for the previous table-using call led by
// this context (ev_io_out, recorded behind that call's launch) -- long past unless that call is still queued behind the caller's stream.
static int stage(cvh_context *lead, size_t host_bytes, size_t dev_bytes)
{
  HIPCHK(lead, hipEventSynchronize(lead->ev_io_out));
  if (lead->h_io_cap < host_bytes) {
    if (lead->h_io) { HIPCHK(lead, hipHostFree(lead->h_io)); lead->h_io = nullptr; lead->h_io_cap = 0; }
    const size_t cap = align_up(host_bytes + host_bytes / 4, 4096);
    HIPCHK(lead, hipHostMalloc(&lead->h_io, cap, hipHostMallocDefault));
    lead->h_io_cap = cap;
  }
  return grow_table(lead, &lead->io_table, dev_bytes);
}

// Before: the leader's stream waits for every member's stream (as cvh_enqueue_steps_batch) and for what the caller has enqueued on
// `stream` so far.  The host waits for nothing.
int open_call(cvh_context *const *ctxs, int n, void *stream)
{
  cvh_context *lead = ctxs[0];
  { const int rc = join_into_leader(ctxs, n); if (rc != CVH_OK) return rc; }
  HIPCHK(lead, hipEventRecord(lead->ev_io_in, (hipStream_t)stream));
  HIPCHK(lead, hipStreamWaitEvent(lead->stream, lead->ev_io_in, 0));
  return CVH_OK;
}

// After: every member's stream, and with to_caller the caller's, waits for the leader's last launch
int close_call(cvh_context *const *ctxs, int n, void *stream, bool to_caller)
{
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipEventRecord(lead->ev_io_out, lead->stream));
  for (int i = 1; i < n; ++i) HIPCHK(ctxs[i], hipStreamWaitEvent(ctxs[i]->stream, lead->ev_io_out, 0));
  if (to_caller) HIPCHK(lead, hipStreamWaitEvent((hipStream_t)stream, lead->ev_io_out, 0));
  return CVH_OK;
}

// sections of the grid: member i owns nblk[i] workgroups behind those of the members before it
unsigned lay_out(CvhIoMember *tab, int n)
{
  unsigned first = 0;
  for (int i = 0; i < n; ++i) { tab[i].first = first; first += tab[i].nblk; }
  return first;
}

int MemberCall::begin(cvh_context *const *ctxs_, int n_, const char *what_, size_t extra_dev, size_t extra_host, bool two_tables)
{
  ctxs = ctxs_; n = n_; what = what_; lead = ctxs[0];
  const size_t tab_bytes = (size_t)n * sizeof(CvhIoMember), tab_pitch = align_up(tab_bytes, 256);
  extra_off = two_tables ? 2 * tab_pitch : tab_pitch;
  dev_bytes = two_tables || extra_dev ? extra_off + extra_dev : tab_bytes;
  host_off = align_up(dev_bytes, 256);
  const int rc = stage(lead, extra_host ? host_off + extra_host : dev_bytes, dev_bytes);
  if (rc != CVH_OK) return rc;
  hb = (unsigned char *)lead->h_io; db = (unsigned char *)lead->io_table.d;
  memset(hb, 0, dev_bytes);
  tab = (CvhIoMember *)hb;
  tab2 = two_tables ? (CvhIoMember *)(hb + tab_pitch) : nullptr;
  for (CvhIoMember *t : {tab, tab2})
    for (int i = 0; t && i < n; ++i) { t[i].n = ctxs[i]->n; t[i].h = ctxs[i]->h; t[i].w = ctxs[i]->w; t[i].C = ctxs[i]->C; }
  return CVH_OK;
}

int MemberCall::arrived(const int *which) const
{
  for (int i = 0; i < n; ++i) {
    if (which && !which[i]) continue;
    const int rc = levelset_arrived(ctxs[i], true);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, ctxs[i]->err);
  }
  return CVH_OK;
}

int MemberCall::upload_again(const CvhIoMember *t) const
{
  HIPCHK(lead, hipMemcpyAsync(db + ((const unsigned char *)t - hb), t, (size_t)n * sizeof(CvhIoMember), hipMemcpyHostToDevice, lead->stream));
  return CVH_OK;
}

// (the event is also the last read of the pinned block; the members' streams wait for the launches on their buffers)
int MemberCall::wait_again(void *stream, bool to_caller) const
{
  const int rc = close_call(ctxs, n, stream, to_caller);
  if (rc != CVH_OK) return rc;
  HIPCHK(lead, hipStreamSynchronize(lead->stream));
  return CVH_OK;
}

// A member receives a fresh level set: it lands in the buffer cvh_set_levelset writes -- the one whose parity is the chain-mode sum
// set's, see levelset_arrived -- and the member's first workgroup clears the device's share of a new run (reset_run_impl): the four run
// words of the state block and the sum set behind the run's own.
void levelset_target(const cvh_context *c, CvhIoMember *m)
{
  m->dst = c->d_u[c->chain_pb & 1];
  m->state_zero = &c->d_state->steps_done;
  m->chain_zero = &c->d_chain->v[(c->chain_pb + 1) & 3][0];
}

// *slot, a workspace of `bytes` that c allocates on first use and keeps; with mirror, the FP64 mirror of an FP32 state is refreshed first
// (the class of a float is the class of its double)
int ensure_workspace(cvh_context *c, void **slot, size_t bytes, const char *name, bool mirror)
{
  if (mirror) { const int rc = ensure_f64_mirror(c); if (rc != CVH_OK) return rc; }
  if (*slot) return CVH_OK;
  const hipError_t e = hipMalloc(slot, bytes);
  if (e == hipSuccess) return CVH_OK;
  *slot = nullptr;
  return fail(c, CVH_ERR_HIP, "hipMalloc of the %s workspace: %s", name, hipGetErrorString(e));
}

// The members' planes were written by the call's launch; its sums come back as the ingest's do (PlaneSums, cvh_host.h)
void PlaneSums::plan(cvh_context *const *ctxs_, int n_)
{
  ctxs = ctxs_; n = n_;
  sums_bytes = (size_t)n * 8 * sizeof(unsigned long long);
  fetch_off.assign((size_t)n, 0);   // inside the host-only part
  fetch_bytes = 0;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    if (stop_norm_exact_on_device(c)) continue;
    fetch_off[i] = fetch_bytes = align_up(fetch_bytes, 256);
    fetch_bytes += c->img_stride * c->C;
    on_host.push_back(i);
  }
}

int PlaneSums::fetch(const MemberCall &call)
{
  cvh_context *lead = call.lead;
  HIPCHK(lead, hipMemcpyAsync(call.hb + call.extra_off, call.db + call.extra_off, sums_bytes, hipMemcpyDeviceToHost, lead->stream));
  for (int i : on_host) {
    const cvh_context *c = ctxs[i];
    HIPCHK(lead, hipMemcpyAsync(call.hb + call.host_off + fetch_off[i], c->d_img_slab, c->img_stride * (c->C - 1) + c->n, hipMemcpyDeviceToHost, lead->stream));
  }
  return CVH_OK;
}

void PlaneSums::arrive(const MemberCall &call)
{
  const unsigned char *const fetched = call.hb + call.host_off;
  const unsigned long long *sums = (const unsigned long long *)(call.hb + call.extra_off);
  // three channels: (sum_k I_k)/3 is rounded per pixel and the reference adds the squares serially (stop_norm_host); members in parallel
  std::vector<double> norm((size_t)n, 0.0);
  auto host_norm = [&](int i) {
    const cvh_context *c = ctxs[i];
    std::vector<const uint8_t *> pl;
    for (int k = 0; k < c->C; ++k) pl.push_back(fetched + fetch_off[i] + (size_t)k * c->img_stride);
    norm[i] = stop_norm_host(pl, c->n);
  };
  const int nthreads = (int)std::min<size_t>(16, on_host.size());
  if (nthreads > 1) {
    std::vector<std::thread> pool;
    try {
      for (int t = 0; t < nthreads; ++t)
        pool.emplace_back([&, t]() { for (size_t q = (size_t)t; q < on_host.size(); q += (size_t)nthreads) host_norm(on_host[q]); });
    } catch (...) {
      for (std::thread &th : pool) th.join();
      pool.clear();
      for (int i : on_host) host_norm(i);   // (no thread to be had: one after the other)
    }
    for (std::thread &th : pool) th.join();
  } else {
    for (int i : on_host) host_norm(i);
  }
  for (int i = 0; i < n; ++i) plane_sums_arrived(ctxs[i], sums + 8 * i, stop_norm_exact_on_device(ctxs[i]) ? nullptr : &norm[i]);
}

// A call whose launch replaces the planes of members 0 .. n_written-1 of ctxs (members n_written .. n_members-1 are only read: their
// iterations stay in flight, ordered before the launch by the stream join).  The written members' iterations in flight are settled, as
// cvh_set_image does; fill(i, m) sets everything of written member i's table entry but `sums`; launch(call) enqueues the kernel on the
// leader's stream and counts it.  Staging: [member table][8 sums per member, zero] uploaded; behind them the planes of the members whose
// stop norm the host takes.  Behind the call's ONE host wait the written members are left as cvh_set_image of those bytes leaves them.
// With payload_bytes, every written member has that many bytes more (a multiple of 16) behind the sums, uploaded with the table in the
// same copy: payload(i, p) fills member i's, and its device address is the entry's src2.
int write_planes(cvh_context *const *ctxs, int n_written, int n_members, const char *what, void *stream,
                 const std::function<void(int, CvhIoMember &)> &fill, const std::function<int(const MemberCall &)> &launch,
                 size_t payload_bytes, const std::function<void(int, void *)> &payload)
{
  HIPCHK(ctxs[0], hipSetDevice(ctxs[0]->device));
  int rc = settle_all(ctxs, n_written, what);
  if (rc != CVH_OK) return rc;
  PlaneSums back;
  back.plan(ctxs, n_written);
  MemberCall call;
  const size_t payload_off = align_up(back.sums_bytes, 256);   // from the call's device extra
  rc = call.begin(ctxs, n_members, what, payload_bytes ? payload_off + (size_t)n_written * payload_bytes : back.sums_bytes, back.fetch_bytes);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n_written; ++i) {
    fill(i, call.tab[i]);
    call.tab[i].sums = back.device_sums(call, i);
    if (!payload_bytes) continue;
    const size_t at = call.extra_off + payload_off + (size_t)i * payload_bytes;
    payload(i, call.hb + at);
    call.tab[i].src2 = call.db + at;
  }
  rc = call.run(stream, false, true, [&]() -> int {   // the sums come back to host fields
    const int rc_launch = launch(call);
    return rc_launch != CVH_OK ? rc_launch : back.fetch(call);
  });
  if (rc != CVH_OK) return rc;
  back.arrive(call);
  return CVH_OK;
}

namespace {

int ingest(cvh_context *const *ctxs, int n, const uint8_t *const *d_imgs, int layout, void *stream, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  if (!d_imgs) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of device pointers is NULL", what);
  if (layout != CVH_LAYOUT_PLANAR && layout != CVH_LAYOUT_INTERLEAVED)
    return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: layout must be CVH_LAYOUT_PLANAR (0) or CVH_LAYOUT_INTERLEAVED (1), got %d", what, layout);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) { rc = pointer_check(ctxs, n, i, d_imgs[i], what); if (rc != CVH_OK) return rc; }
  return write_planes(ctxs, n, n, what, stream, [&](int i, CvhIoMember &m) {
    const cvh_context *c = ctxs[i];
    m.src = d_imgs[i];
    for (int k = 0; k < c->C; ++k) m.plane[k] = c->d_img[k];
    m.interleaved = layout == CVH_LAYOUT_INTERLEAVED;
    m.nblk = cvh_io_blocks(c->n);
  }, [&](const MemberCall &call) -> int { HIPCHK(lead, cvh_launch_io_ingest(call.dtab(), n, call.grid, lead->stream)); return CVH_OK; });
}

}  // namespace

int mask_out(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int invert, void *stream, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  if (!d_masks) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of device pointers is NULL", what);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) { rc = pointer_check(ctxs, n, i, d_masks[i], what); if (rc != CVH_OK) return rc; }
  rc = members_have_levelsets(ctxs, n, what);   // (the arguments first, then the members' state: as the single-context getters)
  if (rc != CVH_OK) return rc;
  rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  MemberCall call;
  rc = call.begin(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    call.tab[i].src = c->d_u[current_buffer(c)];
    call.tab[i].dst = d_masks[i];
    call.tab[i].nblk = cvh_io_blocks(c->n);
  }
  return call.run(stream, true, false, [&]() -> int { HIPCHK(lead, cvh_launch_io_mask(call.dtab(), n, call.grid, invert, lead->stream)); return CVH_OK; });
}

namespace {

// a level set moved in or out: bits is 64 (double) or 32 (float), p aligned to its element
int levelset_args(cvh_context *c, const void *p, int bits, const char *what)
{
  if (bits != 64 && bits != 32) return fail(c, CVH_ERR_ARG, "%s: bits must be 64 or 32, got %d", what, bits);
  if ((uintptr_t)p % (size_t)(bits / 8)) return fail(c, CVH_ERR_ARG, "%s: %p is not aligned to %d bytes", what, p, bits / 8);
  return CVH_OK;
}

}  // namespace

extern "C" int cvh_set_image_device_batch(cvh_context *const *ctxs, int n, const uint8_t *const *d_imgs, int layout, void *stream)
{
  static const char what[] = "cvh_set_image_device_batch";
  return guarded(ctxs, n, what, [&]() { return ingest(ctxs, n, d_imgs, layout, stream, what); });
}

extern "C" int cvh_set_image_device(cvh_context *c, const uint8_t *d_img, int layout, void *stream)
{
  return guarded_one(c, "cvh_set_image_device", [&](const char *what) { return ingest(&c, 1, &d_img, layout, stream, what); });
}

extern "C" int cvh_get_mask_device_batch(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int invert, void *stream)
{
  return mask_out(ctxs, n, d_masks, invert, stream, "cvh_get_mask_device_batch");
}

extern "C" int cvh_get_mask_device(cvh_context *c, uint8_t *d_mask, int invert, void *stream)
{
  if (!c) return CVH_ERR_ARG;
  return mask_out(&c, 1, &d_mask, invert, stream, "cvh_get_mask_device");
}

static int checkerboard_batch(cvh_context *const *ctxs, int n, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  // the h + w sine factors of every distinct shape, from the host's libm: ONE copy with the member table
  std::vector<int> shape_of((size_t)n);
  std::vector<size_t> shape_off;   // inside the extra part
  std::vector<int> shape_first;
  size_t bytes = 0;
  for (int i = 0; i < n; ++i) {
    size_t s = 0;
    while (s < shape_first.size() && !(ctxs[shape_first[s]]->h == ctxs[i]->h && ctxs[shape_first[s]]->w == ctxs[i]->w)) ++s;
    if (s == shape_first.size()) {
      shape_first.push_back(i);
      shape_off.push_back(bytes);
      bytes += ((size_t)ctxs[i]->h + ctxs[i]->w) * sizeof(double);
    }
    shape_of[i] = (int)s;
  }
  MemberCall call;
  rc = call.begin(ctxs, n, what, bytes);
  if (rc != CVH_OK) return rc;
  for (size_t s = 0; s < shape_first.size(); ++s)
    checkerboard_factors(ctxs[shape_first[s]]->h, ctxs[shape_first[s]]->w, (double *)(call.hb + call.extra_off + shape_off[s]));
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    CvhIoMember &m = call.tab[i];
    m.src = call.db + call.extra_off + shape_off[shape_of[i]];
    m.src2 = (const double *)m.src + c->h;
    levelset_target(c, &m);
    m.nblk = cvh_io_checkerboard_blocks(c->h, c->w);
  }
  rc = call.run(nullptr, false, true, [&]() -> int { HIPCHK(lead, cvh_launch_io_checkerboard(call.dtab(), n, call.grid, lead->stream)); return CVH_OK; });
  return rc != CVH_OK ? rc : call.arrived();
}

extern "C" int cvh_init_checkerboard(cvh_context *c)
{
  return guarded_one(c, "cvh_init_checkerboard", [&](const char *what) { return checkerboard_batch(&c, 1, what); });
}

extern "C" int cvh_init_checkerboard_batch(cvh_context *const *ctxs, int n)
{
  static const char what[] = "cvh_init_checkerboard_batch";
  return guarded(ctxs, n, what, [&]() { return checkerboard_batch(ctxs, n, what); });
}

extern "C" int cvh_get_image_device(cvh_context *c, uint8_t *d_img, int layout, void *stream)
{
  static const char what[] = "cvh_get_image_device";
  if (!c) return CVH_ERR_ARG;
  if (layout != CVH_LAYOUT_PLANAR && layout != CVH_LAYOUT_INTERLEAVED)
    return fail(c, CVH_ERR_ARG, "%s: layout must be CVH_LAYOUT_PLANAR (0) or CVH_LAYOUT_INTERLEAVED (1), got %d", what, layout);
  HIPCHK(c, hipSetDevice(c->device));
  int rc = pointer_check(&c, 1, 0, d_img, what);
  if (rc != CVH_OK) return rc;
  if (!c->have_image) return fail(c, CVH_ERR_STATE, "%s: no image set", what);
  if (layout == CVH_LAYOUT_INTERLEAVED && c->C == 3) {
    MemberCall call;
    rc = call.begin(&c, 1, what);
    if (rc != CVH_OK) return rc;
    call.tab->dst = d_img;
    for (int k = 0; k < 3; ++k) call.tab->plane[k] = c->d_img[k];
    call.tab->nblk = cvh_io_blocks(c->n);
    return call.run(stream, true, false, [&]() -> int { HIPCHK(c, cvh_launch_io_image_out3(call.dtab(), 1, call.grid, c->stream)); return CVH_OK; });
  }
  rc = open_call(&c, 1, stream);
  if (rc != CVH_OK) return rc;
  for (int k = 0; k < c->C; ++k)
    HIPCHK(c, hipMemcpyAsync(d_img + (size_t)k * c->n, c->d_img[k], c->n, hipMemcpyDeviceToDevice, c->stream));
  return close_call(&c, 1, stream, true);
}

extern "C" int cvh_set_levelset_device(cvh_context *c, const void *d_u, int bits, void *stream)
{
  static const char what[] = "cvh_set_levelset_device";
  if (!c) return CVH_ERR_ARG;
  int rc = levelset_args(c, d_u, bits, what);
  if (rc != CVH_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  rc = pointer_check(&c, 1, 0, d_u, what);
  if (rc != CVH_OK) return rc;
  rc = settle_all(&c, 1, what);
  if (rc != CVH_OK) return rc;
  const int base = c->chain_pb & 1;   // see levelset_arrived
  rc = open_call(&c, 1, stream);
  if (rc != CVH_OK) return rc;
  if (bits == 64) HIPCHK(c, hipMemcpyAsync(c->d_u[base], d_u, c->n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  else HIPCHK(c, cvh_launch_state_widen((const float *)d_u, c->d_u[base], c->n, c->stream));   // the floats' exact double values
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return levelset_arrived(c);
}

extern "C" int cvh_get_levelset_device(cvh_context *c, void *d_u, int bits, void *stream)
{
  static const char what[] = "cvh_get_levelset_device";
  if (!c) return CVH_ERR_ARG;
  int rc = levelset_args(c, d_u, bits, what);
  if (rc != CVH_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  rc = pointer_check(&c, 1, 0, d_u, what);
  if (rc != CVH_OK) return rc;
  if (!c->have_u) return fail(c, CVH_ERR_STATE, "%s: no level set", what);
  rc = settle_all(&c, 1, what);
  if (rc != CVH_OK) return rc;
  rc = ensure_f64_mirror(c);
  if (rc != CVH_OK) return rc;
  rc = open_call(&c, 1, stream);
  if (rc != CVH_OK) return rc;
  const double *u = c->d_u[current_buffer(c)];
  if (bits == 64) HIPCHK(c, hipMemcpyAsync(d_u, u, c->n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  else HIPCHK(c, cvh_launch_io_narrow(u, (float *)d_u, c->n, c->stream));
  return close_call(&c, 1, stream, true);
}

// Reinitialisation: the level set of every member becomes the signed distance to the pixel-edge front of its mask (reinit_kernels.hip).
// Per member it is cvh_get_levelset -> the header's definition -> cvh_set_levelset: the result lands in the buffer cvh_set_levelset
// writes, and a member whose mask is not uniform then begins a new run through levelset_arrived, the device's half of it done by the
// last launch.  A member with a uniform mask keeps everything, its run state included.
static int reinit_batch(cvh_context *const *ctxs, int n, int *changed, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {   // (member by member: a member without a level set before a later one that is too large)
    rc = members_have_levelsets(ctxs, n, what, i);
    if (rc == CVH_OK) rc = members_distances_fit(ctxs, n, what, i);
    if (rc != CVH_OK) return rc;
  }
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    rc = ensure_workspace(c, &c->d_reinit, cvh_reinit_workspace_bytes(c->h, c->w), "reinitialisation");
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, c->err);
  }
  // staging: [column-pass table][row-pass table][one flag word per member, zero]
  const size_t flag_bytes = (size_t)n * sizeof(unsigned long long);
  MemberCall call;
  rc = call.begin(ctxs, n, what, flag_bytes, 0, true);
  if (rc != CVH_OK) return rc;
  const unsigned long long *flags = (const unsigned long long *)(call.hb + call.extra_off);
  int max_w = 0;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    CvhIoMember &m = call.tab[i];
    m.src = c->d_u[current_buffer(c)];
    levelset_target(c, &m);
    m.plane[0] = (uint8_t *)c->d_reinit;
    m.plane[1] = (uint8_t *)c->d_reinit + cvh_reinit_bits_bytes(c->h, c->w);
    m.sums = (unsigned long long *)(call.db + call.extra_off) + i;
    call.tab2[i] = m;
    m.nblk = cvh_reinit_column_blocks(c->h, c->w);
    call.tab2[i].nblk = cvh_reinit_row_blocks(c->h);
    max_w = std::max(max_w, c->w);
  }
  rc = call.run(nullptr, false, true, [&]() -> int {   // the ONE host wait of the call: which members changed
    HIPCHK(lead, cvh_launch_reinit(call.dtab(), call.grid, call.dtab2(), call.grid2, n, max_w, lead->stream));
    ++g_launches[kReinitLaunchSets];
    HIPCHK(lead, hipMemcpyAsync((void *)flags, call.db + call.extra_off, flag_bytes, hipMemcpyDeviceToHost, lead->stream));
    HIPCHK(lead, hipEventRecord(lead->ev1, lead->stream));
    return CVH_OK;
  }, lead->ev0);   // (ev0 is free: settle closed any timed run)
  if (rc != CVH_OK) return rc;
  HIPCHK(lead, hipEventElapsedTime(&lead->last_reinit_ms, lead->ev0, lead->ev1));
  std::unique_ptr<int[]> own;
  if (!changed) { own.reset(new int[n]); changed = own.get(); }
  for (int i = 0; i < n; ++i) changed[i] = (flags[i] & 3) == 3 ? 1 : 0;
  return call.arrived(changed);
}

extern "C" int cvh_reinit_batch(cvh_context *const *ctxs, int n, int *changed)
{
  static const char what[] = "cvh_reinit_batch";
  return guarded(ctxs, n, what, [&]() { return reinit_batch(ctxs, n, changed, what); });
}

extern "C" int cvh_reinit(cvh_context *c, int *changed)
{
  return guarded_one(c, "cvh_reinit", [&](const char *what) { return reinit_batch(&c, 1, changed, what); });
}
