// edge_run.hip — host side of the edge-plane calls (include/chanvese_hip.h, "Edge-weighted length"; kernels in edge_kernels.hip): a
// context's edge plane set from and read into host or device memory, and built from the planes of a source context by the Sobel map,
// N pairs in one launch on the member table.  The plane is the context's own buffer, allocated by the first call that writes it; no
// image or level-set call touches it, and cvh_geodesic_run* only reads it.
#include "cvh_host.h"

namespace {

int edge_plane(cvh_context *c)
{
  if (c->d_gq) return CVH_OK;
  const hipError_t e = hipMalloc((void **)&c->d_gq, c->n * sizeof(uint16_t));
  if (e == hipSuccess) return CVH_OK;
  c->d_gq = nullptr;
  return fail(c, CVH_ERR_HIP, "hipMalloc of the edge plane: %s", hipGetErrorString(e));
}

// den = ((64 C) K) K, taken once on the host: 64 turns the Sobel sums into a unit-spacing gradient, C averages the channels
bool edge_den(int channels, double K, double *den)
{
  if (!std::isfinite(K) || K <= 0.0) return false;
  *den = ((64.0 * channels) * K) * K;
  return std::isfinite(*den);
}

// all = the n destinations, then every source that is not a destination: the call's member list, each context once
int edge_check(cvh_context *const *dsts, cvh_context *const *srcs, int n, const double *K, const char *what, std::vector<cvh_context *> *all,
               std::vector<double> *den)
{
  if (!dsts || !srcs || n < 1)
    return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: empty pair list (dsts = %p, srcs = %p, n = %d)", what, (const void *)dsts, (const void *)srcs, n);
  for (int i = 0; i < n; ++i)
    if (!dsts[i] || !srcs[i]) return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: pair %d: the %s context is NULL", what, i, dsts[i] ? "source" : "destination");
  all->assign(dsts, dsts + n);
  for (int i = 0; i < n; ++i)
    if (std::find(all->begin(), all->end(), srcs[i]) == all->end()) all->push_back(srcs[i]);
  cvh_context *const *ctxs = all->data();
  const int m = (int)all->size();
  if (!K) return batch_fail(ctxs, m, CVH_ERR_ARG, "%s: K is NULL", what);
  den->assign((size_t)n, 0.0);
  for (int i = 0; i < n; ++i) {
    const cvh_context *d = dsts[i], *s = srcs[i];
    for (int j = 0; j < i; ++j)
      if (dsts[j] == d) return batch_fail(ctxs, m, CVH_ERR_ARG, "%s: pair %d: its destination context is also pair %d's (a destination may be listed once)", what, i, j);
    for (const cvh_context *x : {d, s})
      if (x->device != ctxs[0]->device)
        return batch_fail(ctxs, m, CVH_ERR_ARG, "%s: pair %d: its %s context is on device %d, pair 0's on device %d", what, i, x == d ? "destination" : "source",
                          x->device, ctxs[0]->device);
    if (d->h != s->h || d->w != s->w)
      return batch_fail(ctxs, m, CVH_ERR_ARG, "%s: pair %d: the destination of a %d x %d source must be %d x %d too, got %d x %d", what, i, s->h, s->w, s->h,
                        s->w, d->h, d->w);
    if (!edge_den(s->C, K[i], &(*den)[i]))
      return batch_fail(ctxs, m, CVH_ERR_ARG, "%s: pair %d: K = %g, must be finite and positive with a finite 64 C K^2", what, i, K[i]);
  }
  for (int i = 0; i < n; ++i)
    if (!srcs[i]->have_image) return batch_fail(ctxs, m, CVH_ERR_STATE, "%s: pair %d: the source context has no image (call cvh_set_image first)", what, i);
  return CVH_OK;
}

int edge_map_batch(cvh_context *const *dsts, cvh_context *const *srcs, int n, const double *K, const char *what)
{
  std::vector<cvh_context *> all;
  std::vector<double> den;
  int rc = edge_check(dsts, srcs, n, K, what, &all, &den);
  if (rc != CVH_OK) return rc;
  cvh_context *const *ctxs = all.data();
  const int m = (int)all.size();
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) {
    rc = edge_plane(dsts[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, m, rc, "%s: pair %d: %s", what, i, dsts[i]->err);
  }
  MemberCall call;
  rc = call.begin(ctxs, m, what, (size_t)n * sizeof(double));
  if (rc != CVH_OK) return rc;
  memcpy(call.hb + call.extra_off, den.data(), (size_t)n * sizeof(double));
  for (int i = 0; i < n; ++i) {   // (the table's first n entries -- the destinations' -- are the kernel's members)
    CvhIoMember &e = call.tab[i];
    e.src = srcs[i]->d_img_slab;
    e.src_stride = srcs[i]->img_stride;
    e.w2 = srcs[i]->C;
    e.dst = dsts[i]->d_gq;
    e.nblk = cvh_edge_blocks(dsts[i]->n);
  }
  rc = call.run(nullptr, false, true, [&]() -> int {
    HIPCHK(lead, cvh_launch_edge_map(call.dtab(), (const double *)(call.db + call.extra_off), n, call.grid, lead->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) dsts[i]->have_gq = true;
  return CVH_OK;
}

}  // namespace

extern "C" int cvh_set_edge_map(cvh_context *ctx, const uint16_t *host)
{
  return guarded_one(ctx, "cvh_set_edge_map", [&](const char *what) -> int {
    if (!host) return fail(ctx, CVH_ERR_ARG, "%s: the edge map is NULL", what);
    for (size_t q = 0; q < ctx->n; ++q)
      if (host[q] > CVH_EDGE_ONE) return fail(ctx, CVH_ERR_ARG, "%s: value %u at pixel %zu, an edge weight is 0 .. %d", what, (unsigned)host[q], q, CVH_EDGE_ONE);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = edge_plane(ctx);
    if (rc != CVH_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_gq, host, ctx->n * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_gq = true;
    return CVH_OK;
  });
}

extern "C" int cvh_get_edge_map(cvh_context *ctx, uint16_t *host)
{
  return guarded_one(ctx, "cvh_get_edge_map", [&](const char *what) -> int {
    if (!host) return fail(ctx, CVH_ERR_ARG, "%s: the output is NULL", what);
    if (!ctx->have_gq) return fail(ctx, CVH_ERR_STATE, "%s: the context has no edge plane (call cvh_set_edge_map or cvh_edge_map first)", what);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(host, ctx->d_gq, ctx->n * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CVH_OK;
  });
}

// ordered behind `stream` and in front of what is enqueued on it later; no host wait
extern "C" int cvh_set_edge_map_device(cvh_context *ctx, const uint16_t *d_gq, void *stream)
{
  return guarded_one(ctx, "cvh_set_edge_map_device", [&](const char *what) -> int {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = element_pointer_check(&ctx, 1, 0, d_gq, sizeof(uint16_t), what);
    if (rc != CVH_OK) return rc;
    rc = edge_plane(ctx);
    if (rc != CVH_OK) return rc;
    rc = open_call(&ctx, 1, stream);
    if (rc != CVH_OK) return rc;
    HIPCHK(ctx, cvh_launch_edge_clamp(d_gq, ctx->d_gq, ctx->n, ctx->stream));
    rc = close_call(&ctx, 1, stream, true);
    if (rc == CVH_OK) ctx->have_gq = true;   // (only once the copy is ordered against the caller's stream)
    return rc;
  });
}

extern "C" int cvh_get_edge_map_device(cvh_context *ctx, uint16_t *d_gq, void *stream)
{
  return guarded_one(ctx, "cvh_get_edge_map_device", [&](const char *what) -> int {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = element_pointer_check(&ctx, 1, 0, d_gq, sizeof(uint16_t), what);
    if (rc != CVH_OK) return rc;
    if (!ctx->have_gq) return fail(ctx, CVH_ERR_STATE, "%s: the context has no edge plane (call cvh_set_edge_map or cvh_edge_map first)", what);
    rc = open_call(&ctx, 1, stream);
    if (rc != CVH_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_gq, ctx->d_gq, ctx->n * sizeof(uint16_t), hipMemcpyDeviceToDevice, ctx->stream));
    return close_call(&ctx, 1, stream, true);
  });
}

extern "C" int cvh_edge_map_batch(cvh_context *const *dsts, cvh_context *const *srcs, int n, const double *K)
{
  static const char what[] = "cvh_edge_map_batch";
  return guarded(nullptr, 0, what, [&]() { return edge_map_batch(dsts, srcs, n, K, what); });
}

extern "C" int cvh_edge_map(cvh_context *dst, cvh_context *src, double K)
{
  static const char what[] = "cvh_edge_map";
  return guarded(nullptr, 0, what, [&]() { return edge_map_batch(&dst, &src, 1, &K, what); });
}
