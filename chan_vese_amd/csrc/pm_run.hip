// pm_run.hip — the Perona-Malik pre-smoother: the resident and per-launch flows of one context (cvh_perona_malik) and the batch that
// packs the planes of N contexts into shared resident launches (cvh_perona_malik_batch).
#include "cvh_host.h"

// Perona-Malik on a resident plane (pm_resident_kernel.hip): any channel count (the planes are smoothed one after the other), both
// arithmetic flavours; the same tiles as the CSV kernel.
// workgroups of pm_resident_kernel the device holds at once, at most one per CU and CVH_RESIDENT_MAX_TILES (0: no cooperative launch)
static int pm_resident_tiles_cap(cvh_context *c)
{
  if (c->pm_resident_cap < 0) c->pm_resident_cap = launches_cooperatively(c) ? cvh_pm_resident_blocks_per_cu() * c->num_cus : 0;
  if (c->pm_resident_cap <= 0) return 0;
  int cap = c->pm_resident_cap < CVH_RESIDENT_MAX_TILES ? c->pm_resident_cap : CVH_RESIDENT_MAX_TILES;
  if (cap > c->num_cus) cap = c->num_cus;                      // one workgroup per CU
  return cap;
}

static bool pm_resident_geometry(cvh_context *c, ResidentGeom *rg)
{
  if ((c->w & 1) || c->w < 16 || c->h < 16) return false;
  const int cap = pm_resident_tiles_cap(c);
  if (cap <= 0) return false;
  const int tc = (c->w + cvh_resident_tile_w() - 1) / cvh_resident_tile_w();
  // tiles of 8 x band rows x 128 columns, every wave a band of exactly 2, 4, 8 or 16 rows: the shortest bands whose tiles the CUs hold at once
  // (more CUs at work); the last tile row of the image may be shorter, but holds at least the two rows a border piece needs
  for (int nr = 2; nr <= 16; nr *= 2) {
    const int th = 8 * nr, tr = (c->h + th - 1) / th;
    if (tr * tc > cap) continue;
    if (c->h - (tr - 1) * th < 2) continue;
    rg->tr = tr; rg->tc = tc; rg->band = nr;
    return true;
  }
  return false;
}

extern "C" int cvh_pm_trip_count(double L, double T)
{
  int n = 0;
  for (double t = 0; t < T; t += L) {  // src/main.cpp:498: the counter itself is a double
    if (++n == INT_MAX) break;
    if (!(L > 0)) break;               // L == 0 would never terminate; one step is what T >= L allows
  }
  return n;
}

// "pm_kernel" = -1: the resident kernel pays ~25 us per cooperative launch that the per-launch flow does not, and gains 0.9 us per step
// on small planes, 1.6 at 1024^2, 4 at 2048^2 (tools/pm_flows.py): runs shorter than this keep the per-launch flow
static int pm_resident_min_trips(size_t n) { return n >= ((size_t)3 << 20) ? 8 : (n >= ((size_t)1 << 20) ? 16 : 32); }

// pm_resident_kernel's border buffer: room for CVH_RESIDENT_MAX_TILES tiles per step parity
static int ensure_pm_halo(cvh_context *c)
{
  if (c->d_pm_halo) return CVH_OK;
  const size_t bytes = (size_t)2 * CVH_RESIDENT_MAX_TILES * cvh_pm_resident_halo_doubles() * sizeof(double);
  HIPCHK(c, hipMalloc((void **)&c->d_pm_halo, bytes));
  HIPCHK(c, hipMemset(c->d_pm_halo, 0, bytes));            // tag 0: matches no launch
  return CVH_OK;
}

// cvh_perona_malik's argument checks (src/main.cpp:863-867, and K != 0), for a context or a batch member: CVH_OK, or CVH_ERR_ARG with the
// refusal in msg (the K check's behind k_prefix)
static int pm_check_args(double K, double L, double T, const char *k_prefix, char *msg, size_t cap)
{
  if (L > 0.25 || L < 0) snprintf(msg, cap, "The Laplacian coefficient in Perona-Malik segmentation must be between 0 and 0.25.");
  else if (T < L) snprintf(msg, cap, "The segmentation duration must exceed the value of Laplacian coefficient, %f.", L);
  else if (K == 0) snprintf(msg, cap, "%sedge coefficient K must be non-zero", k_prefix);
  else return CVH_OK;
  return CVH_ERR_ARG;
}

static const char kPmNeedsResident[] =
    "pm_kernel 4 (resident plane) needs an even width, >= 16 rows and columns, and a plane that fits the LDS of the CUs";

// the FP64 ping-pong planes a channel is smoothed in
static int ensure_pm_planes(cvh_context *c)
{
  for (int k = 0; k < 2; ++k)
    if (!c->d_pm[k]) HIPCHK(c, hipMalloc((void **)&c->d_pm[k], c->n * sizeof(double)));
  return CVH_OK;
}

// Perona-Malik with the plane resident in LDS: per channel uint8 -> FP64 plane, ONE cooperative launch per chunk of time steps,
// FP64 -> uint8 (round-half-even, :551) behind the last step.
static int pm_run_resident(cvh_context *c, const CvhPmArgs &base, const ResidentGeom &rg, int trips)
{
  { const int rc = ensure_resident_buffers(c); if (rc != CVH_OK) return rc; }
  CvhPmArgs a = base;
  a.tiles_x = rg.tc; a.tiles_y = rg.tr; a.res_band_rows = rg.band;
  a.res_prio = c->res_prio;
  a.resident = c->d_resident;
  { const int rc = ensure_pm_halo(c); if (rc != CVH_OK) return rc; }
  a.res_halo = c->d_pm_halo;
  a.res_poll_cap = kPmPollCap;
  a.dbg_times = c->d_dbg;
  constexpr int kMaxPerLaunch = kPmMaxPerLaunch;
  {
    CvhLaunchNote nb{};
    CvhPmArgs pa = a; pa.note = &nb; pa.res_steps = trips;
    (void)cvh_launch_pm_resident(pa, c->stream);
    snprintf(c->pm_desc, sizeof(c->pm_desc), "kernel=%s grid=%u block=%u lds_bytes=%u steps_per_launch=%d tiles_y=%d tiles_x=%d launches=%d graph_launches=0 trips=%d planes=%d",
             nb.name, nb.grid, nb.block, nb.lds, trips < kMaxPerLaunch ? trips : kMaxPerLaunch, rg.tr, rg.tc, (trips + kMaxPerLaunch - 1) / kMaxPerLaunch, trips, c->C);
  }
  HIPCHK(c, hipMemsetAsync(c->d_resident, 0, CVH_RESIDENT_C1_BYTES, c->stream));
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  for (int k = 0; k < c->C; ++k) {
    HIPCHK(c, cvh_launch_pm_load(c->d_img[k], c->d_pm[0], c->n, c->stream));
    int cur = 0;
    for (int t = 0; t < trips;) {
      const int n = trips - t < kMaxPerLaunch ? trips - t : kMaxPerLaunch;
      CvhPmArgs pa = a;
      pa.in = c->d_pm[cur]; pa.out = c->d_pm[cur ^ 1]; pa.res_steps = n;
      pa.res_serial = ++c->pm_res_serial;        // border entries carry {serial, step}: nothing an earlier launch left can match
      HIPCHK(c, cvh_launch_pm_resident(pa, c->stream));
      cur ^= 1;
      t += n;
    }
    HIPCHK(c, cvh_launch_pm_store(c->d_pm[cur], c->d_img[k], c->n, c->stream));
    c->pm_plane = cur;
  }
  return CVH_OK;
}

// Perona-Malik with a launch per time step, or per two (pm_wave_k2_kernel.hip), from the base arguments `a`; up to the launches of the last
// plane (cvh_perona_malik records the end of the run).
static int pm_run_per_launch(cvh_context *c, CvhPmArgs a, int trips)
{
  // two time steps per launch (pm_wave_k2_kernel.hip): planes that fit the caches, where a step is launch / latency bound
  // (a 2-pixel-per-lane 1-step kernel was the default from 12 Mpixel on in round 1: 48.4 us/step at 4096^2 against 39.3 for the 2-step
  // kernel -- tools/experiments/pruned_flavours/pm_wave2_kernel.hip)
  const bool pm_k2 = trips >= 2 && c->n < ((size_t)1 << 28) && (c->pm_kernel == 3 || c->pm_kernel == -1);
  const bool pm_wave = c->pm_kernel != 0;
  CvhPmArgs a2 = a;      // geometry of the 2-step kernel (the odd last step runs the 1-step wave kernel)
  if (pm_k2) {
    a2.tiles_x = (c->w + cvh_pm_wave_k2_cols() - 1) / cvh_pm_wave_k2_cols();
    int sr = c->pm_strip_rows;
    if (sr <= 0) {
      // ~51 strips whatever the size (measured, us/step: 1024^2: 16 rows 6.3, 24 rows 6.05, 32 rows 6.7; 2048^2: 16 13.0, 24 13.2,
      // 32 13.3, 40 12.55, 48 13.5, 64 15.5; 4096^2: 48 40.1, 64 39.8, 80 38.2-39.3, 104 38.6, 128 41.9, 160 39.9, 200 44.6)
      sr = (c->h + 50) / 51;
      sr = ((sr + 4) / 8) * 8;   // nearest multiple of 8: the row loop is unrolled by 8
      if (sr < 16) sr = 16;      // every strip pays 5 extra stage-1 rows
    }
    a2.strip_rows = sr;
  }
  if (pm_wave) {
    a.tiles_x = (c->w + cvh_pm_wave_cols() - 1) / cvh_pm_wave_cols();
    int sr = c->pm_strip_rows;
    if (sr <= 0) {  // ~3 waves per SIMD resident
      int nstrips = (c->num_cus * 3) / ((a.tiles_x + 3) / 4);
      if (nstrips < 1) nstrips = 1;
      sr = (c->h + nstrips - 1) / nstrips;
      sr = ((sr + 3) / 8) * 8;  // nearest multiple of the 8-row loop body; measured best: 8 / 8-16 / 24 rows at 512^2 / 1024^2 / 2048^2
      if (sr < 8) sr = 8;
    }
    a.strip_rows = sr;
  } else {
    cvh_pm_grid(c->h, c->w, &a.tiles_x, &a.tiles_y);
  }
  const int kind = pm_wave ? 1 : 0;
  auto launch_pm = [&](const CvhPmArgs &pa) -> hipError_t {
    return pm_wave ? cvh_launch_pm_wave(pa, c->stream) : cvh_launch_pm_step(pa, c->stream);
  };
  const int per_launch = pm_k2 ? 2 : 1;   // time steps per launch of the bulk kernel
  auto launch_bulk = [&](int from, CvhLaunchNote *note = nullptr) -> hipError_t {
    if (!pm_k2) { CvhPmArgs pa = a; pa.in = c->d_pm[from]; pa.out = c->d_pm[from ^ 1]; pa.note = note; return launch_pm(pa); }
    CvhPmArgs pa = a2; pa.in = c->d_pm[from]; pa.out = c->d_pm[from ^ 1]; pa.note = note;
    return cvh_launch_pm_wave_k2(pa, c->stream);
  };
  {   // what this call launches, for cvh_launch_info (filled by the launch sites themselves)
    CvhLaunchNote nb{}, no{};
    (void)launch_bulk(0, &nb);
    const bool odd = trips % per_launch != 0;
    if (odd) { CvhPmArgs pa = a; pa.in = c->d_pm[0]; pa.out = c->d_pm[1]; pa.note = &no; (void)launch_pm(pa); }
    const bool graphed = c->use_graph && trips >= kGraphSteps * per_launch;
    snprintf(c->pm_desc, sizeof(c->pm_desc),
             "kernel=%s grid=%u block=%u steps_per_launch=%d strip_rows=%d launches=%d%s%s graph_launches=%d trips=%d planes=%d",
             nb.name, nb.grid, nb.block, per_launch, pm_k2 ? a2.strip_rows : a.strip_rows, trips / per_launch,
             odd ? " last_step_kernel=" : "", odd ? no.name : "", graphed ? kGraphSteps : 0, trips, c->C);
  }
  // kGraphSteps steps as one hipGraph, as for the CSV step: a graph node costs 1.6 us against 2.8 us for a stream launch
  // (tools/launch_probe.hip) and a 2048^2 step is only ~13 us.  The graph always starts from d_pm[0] (16 is even).
  if (c->use_graph && trips >= kGraphSteps * per_launch) {
    CvhPmArgs key = pm_k2 ? a2 : a;
    key.in = c->d_pm[0]; key.out = c->d_pm[1];
    if (!c->pm_graph || c->pm_graph_kind != kind + 10 * pm_k2 || memcmp(&key, &c->pm_graph_key, sizeof(key))) {
      if (c->pm_graph) { (void)hipGraphExecDestroy(c->pm_graph); c->pm_graph = nullptr; }
      const char *const capture_failed = "cvh_perona_malik: graph capture failed (%s)";
      const int rc = capture_graph(c, &c->pm_graph, [&] {
        hipError_t e = hipSuccess;
        for (int t = 0; t < kGraphSteps && e == hipSuccess; ++t) e = launch_bulk(t & 1);
        return e == hipSuccess ? CVH_OK : fail(c, CVH_ERR_HIP, capture_failed, hipGetErrorString(e));
      }, capture_failed);
      if (rc != CVH_OK) return rc;
      c->pm_graph_key = key; c->pm_graph_kind = kind + 10 * pm_k2;
    }
  }
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  if (trips > 0) {
    for (int k = 0; k < c->C; ++k) {
      HIPCHK(c, cvh_launch_pm_load(c->d_img[k], c->d_pm[0], c->n, c->stream));
      int cur = 0, t = 0;
      for (; c->use_graph && c->pm_graph && trips - t >= kGraphSteps * per_launch; t += kGraphSteps * per_launch) HIPCHK(c, hipGraphLaunch(c->pm_graph, c->stream));
      for (; trips - t >= per_launch; t += per_launch) { HIPCHK(c, launch_bulk(cur)); cur ^= 1; }
      for (; t < trips; ++t) {   // the odd last step of the 2-step flavour
        a.in = c->d_pm[cur]; a.out = c->d_pm[cur ^ 1];
        HIPCHK(c, launch_pm(a));
        cur ^= 1;
      }
      HIPCHK(c, cvh_launch_pm_store(c->d_pm[cur], c->d_img[k], c->n, c->stream));
      c->pm_plane = cur;
    }
  }
  return CVH_OK;
}

extern "C" int cvh_perona_malik(cvh_context *c, double K, double L, double T)
{
  if (!c) return CVH_ERR_ARG;
  if (!c->have_image) return fail(c, CVH_ERR_STATE, "cvh_perona_malik: no image set");
  char msg[256];
  if (pm_check_args(K, L, T, "cvh_perona_malik: ", msg, sizeof(msg)) != CVH_OK) return fail(c, CVH_ERR_ARG, "%s", msg);
  HIPCHK(c, hipSetDevice(c->device));
  // CSV work that was enqueued and never synchronised is closed first, as cvh_set_image does: the resident Perona-Malik flow clears the
  // shared CvhResident block (the error word of an unsynchronised csv_resident_kernel launch with it) and reuses ev0 / ev1.
  int rc = settle(c);
  if (rc == CVH_OK) rc = ensure_pm_planes(c);
  if (rc != CVH_OK) return rc;
  const int trips = cvh_pm_trip_count(L, T);
  CvhPmArgs a;
  memset(&a, 0, sizeof(a));
  a.h = c->h; a.w = c->w; a.K2 = K * K; a.L = L;
  a.invK2 = 1.0 / (K * K); a.L4 = L / 4; a.fast = use_fast(c) ? 1 : 0;
  a.pol = (c->wave_pol >= 0 ? (c->wave_pol == 1) : ((double)c->n * 16.0 <= 300e6 ? 1 : 0));
  // A plane whose FP64 state fits the chip's LDS stays there for the whole run (pm_resident_kernel.hip): one cooperative launch per
  // channel, the tiles' borders cross workgroups, nothing else moves.
  ResidentGeom rg;
  const bool want = c->pm_kernel == 4 || (c->pm_kernel == -1 && c->pm_strip_rows == 0 && trips >= pm_resident_min_trips(c->n));
  const bool resident = want && trips > 0 && pm_resident_geometry(c, &rg);
  if (!resident && c->pm_kernel == 4 && trips > 0) return fail(c, CVH_ERR_ARG, "%s", kPmNeedsResident);
  // d_pm[] is overwritten from here on: the flow records the plane its last pm_store reads (cvh_debug_pm_plane).  (T = L = 0 is the one
  // accepted call with no trip: it touches nothing, the plane of the last call that stepped stays.)
  if (trips > 0) c->pm_plane = -1;
  rc = resident ? pm_run_resident(c, a, rg, trips) : pm_run_per_launch(c, a, trips);
  if (rc != CVH_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  if (resident) HIPCHK(c, hipMemcpyAsync(c->h_resident, c->d_resident, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->last_pm_ms = ms;
  planes_changed(c);   // the stop norm and the region means are taken again
  if (resident && c->h_resident[0]) {
    c->h_resident[0] = 0;
    c->pm_plane = -1;
    return fail(c, CVH_ERR_HIP, "cvh_perona_malik: a wait of the resident kernel gave up (a workgroup was not resident, or a fault); the planes are undefined");
  }
  return CVH_OK;
}

// ---- Perona-Malik batch: the planes of N contexts share cooperative launches of pm_resident_batch_kernel (include/chanvese_hip.h) ----
// A launch holds planes of one round (channel k of every member that has one) and one arithmetic flavour; each plane is cut into tiles of
// 8 x nr rows x 128 columns, nr common to the launch (a template parameter), and keeps its own K, L and step count.
struct PmBatchLaunch { int round = 0, fast = 0, nr = 0, ntiles = 0; std::vector<int> members; };

// tiles of c's plane in tiles of 8 x nr rows (0: the last tile row would hold fewer than the two rows a border piece needs)
static int pm_batch_tiles(const cvh_context *c, int nr)
{
  const int th = 8 * nr, tr = (c->h + th - 1) / th, tc = (c->w + cvh_resident_tile_w() - 1) / cvh_resident_tile_w();
  return c->h - (tr - 1) * th < 2 ? 0 : tr * tc;
}

// first fit: member i's plane joins launch b if some band nr lets all of b's planes and it fit `cap` tiles; b takes the smallest such nr
static bool pm_batch_add(PmBatchLaunch &b, cvh_context *const *ctxs, int i, int cap)
{
  for (int nr = 2; nr <= 16; nr *= 2) {
    int tot = pm_batch_tiles(ctxs[i], nr);
    for (size_t q = 0; q < b.members.size() && tot > 0; ++q) {
      const int t = pm_batch_tiles(ctxs[b.members[q]], nr);
      tot = t > 0 ? tot + t : 0;
    }
    if (tot <= 0 || tot > cap) continue;
    b.nr = nr; b.ntiles = tot;
    b.members.push_back(i);
    return true;
  }
  return false;
}

extern "C" int cvh_perona_malik_batch(cvh_context *const *ctxs, int n, const double *K, const double *L, const double *T)
{
  int rc = members_check(ctxs, n, "batch", kMembersWithImage);
  if (rc != CVH_OK) return rc;
  if (!K || !L || !T) return batch_fail(ctxs, n, CVH_ERR_ARG, "pm batch: K, L and T must each hold the n = %d members' values", n);
  char msg[256];
  for (int i = 0; i < n; ++i)   // cvh_perona_malik's own checks, every member before anything runs
    if (pm_check_args(K[i], L[i], T[i], "", msg, sizeof(msg)) != CVH_OK) return batch_fail(ctxs, n, CVH_ERR_ARG, "pm batch: member %d: %s", i, msg);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  // which members are fused: the automatic or the resident choice, no strip rows, a plane that qualifies on its own, one launch per plane
  int cap = pm_resident_tiles_cap(lead);
  const int bcap = cvh_pm_resident_batch_blocks_per_cu() * lead->num_cus;
  if (bcap < cap) cap = bcap;
  std::vector<int> trips((size_t)n), fused((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    trips[i] = cvh_pm_trip_count(L[i], T[i]);
    ResidentGeom rg;
    const bool fits = trips[i] > 0 && pm_resident_geometry(c, &rg);
    if (c->pm_kernel == 4 && trips[i] > 0 && !fits) return batch_fail(ctxs, n, CVH_ERR_ARG, "pm batch: member %d: %s", i, kPmNeedsResident);
    PmBatchLaunch probe;
    fused[i] = fits && (c->pm_kernel == -1 || c->pm_kernel == 4) && c->pm_strip_rows == 0 && trips[i] <= kPmMaxPerLaunch && pm_batch_add(probe, ctxs, i, cap);
  }
  // CSV work that was enqueued and never synchronised is closed first, as cvh_perona_malik does
  for (int i = 0; i < n; ++i) {
    rc = settle(ctxs[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "pm batch: member %d: %s", i, ctxs[i]->err);
  }
  // packing (include/chanvese_hip.h): round k = channel k; inside a round FAST planes, then STRICT ones; first fit in member order
  std::vector<PmBatchLaunch> launches;
  int rounds = 0;
  for (int i = 0; i < n; ++i) if (fused[i] && ctxs[i]->C > rounds) rounds = ctxs[i]->C;
  for (int k = 0; k < rounds; ++k)
    for (int f = 1; f >= 0; --f) {
      const size_t first = launches.size();
      for (int i = 0; i < n; ++i) {
        if (!fused[i] || ctxs[i]->C <= k || (use_fast(ctxs[i]) ? 1 : 0) != f) continue;
        bool placed = false;
        for (size_t b = first; b < launches.size() && !placed; ++b) placed = pm_batch_add(launches[b], ctxs, i, cap);
        if (!placed) {
          launches.emplace_back();
          launches.back().round = k; launches.back().fast = f;
          (void)pm_batch_add(launches.back(), ctxs, i, cap);   // (fits alone: checked above)
        }
      }
    }
  if (!launches.empty()) {
    for (int i = 0; i < n; ++i) {
      cvh_context *c = ctxs[i];
      if (!fused[i]) continue;
      rc = ensure_pm_planes(c);
      if (rc != CVH_OK) return rc;
    }
    rc = ensure_resident_buffers(lead);
    if (rc == CVH_OK) rc = ensure_pm_halo(lead);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "pm batch: member 0: %s", lead->err);
    // the tables of every launch in one upload: [planes][map][load planes][store planes] per launch
    struct Off { size_t planes, map, io_load, io_store; };
    std::vector<Off> off(launches.size());
    size_t bytes = 0;
    auto take = [&](size_t sz) { const size_t o = (bytes + 255) & ~(size_t)255; bytes = o + sz; return o; };
    for (size_t b = 0; b < launches.size(); ++b) {
      const size_t np = launches[b].members.size();
      off[b].planes = take(np * sizeof(CvhPmBatchPlane));
      off[b].map = take((size_t)launches[b].ntiles * sizeof(unsigned));
      off[b].io_load = take(np * sizeof(CvhPmIoPlane));
      off[b].io_store = take(np * sizeof(CvhPmIoPlane));
    }
    std::vector<unsigned char> img(bytes, 0);
    for (size_t b = 0; b < launches.size(); ++b) {
      const PmBatchLaunch &bl = launches[b];
      const unsigned serial = ++lead->pm_res_serial;   // border entries carry {serial, step}: nothing an earlier launch left can match
      int base = 0;
      for (size_t q = 0; q < bl.members.size(); ++q) {
        const int i = bl.members[q];
        cvh_context *c = ctxs[i];
        CvhPmBatchPlane pl;
        memset(&pl, 0, sizeof(pl));
        CvhPmArgs &a = pl.a;
        a.in = c->d_pm[0]; a.out = c->d_pm[1];
        a.h = c->h; a.w = c->w;
        a.tiles_x = (c->w + cvh_resident_tile_w() - 1) / cvh_resident_tile_w();
        a.tiles_y = (c->h + 8 * bl.nr - 1) / (8 * bl.nr);
        a.K2 = K[i] * K[i]; a.L = L[i];
        a.invK2 = 1.0 / (K[i] * K[i]); a.L4 = L[i] / 4; a.fast = bl.fast;
        a.resident = lead->d_resident; a.res_halo = lead->d_pm_halo; a.res_serial = serial;
        a.res_steps = trips[i]; a.res_band_rows = bl.nr; a.res_prio = c->res_prio; a.res_poll_cap = kPmPollCap;
        pl.tile_base = base;
        memcpy(img.data() + off[b].planes + q * sizeof(CvhPmBatchPlane), &pl, sizeof(pl));
        unsigned *map = (unsigned *)(img.data() + off[b].map);
        for (int t = 0; t < a.tiles_x * a.tiles_y; ++t) map[base + t] = (unsigned)q;
        base += a.tiles_x * a.tiles_y;
        const CvhPmIoPlane ld = {c->d_img[bl.round], c->d_pm[0], (unsigned long long)c->n};   // channel `round` into the launch's input
        const CvhPmIoPlane st = {c->d_img[bl.round], c->d_pm[1], (unsigned long long)c->n};   // its output back (round-half-even, :551)
        memcpy(img.data() + off[b].io_load + q * sizeof(CvhPmIoPlane), &ld, sizeof(ld));
        memcpy(img.data() + off[b].io_store + q * sizeof(CvhPmIoPlane), &st, sizeof(st));
      }
      if (base != bl.ntiles) return batch_fail(ctxs, n, CVH_ERR_STATE, "pm batch: internal error: launch %d has %d tiles, packed for %d", (int)b, base, bl.ntiles);
    }
    rc = grow_table(lead, &lead->pm_batch, bytes);
    // every member's stream joins the leader's; all launches run there
    if (rc == CVH_OK) rc = join_into_leader(ctxs, n, fused.data());
    if (rc != CVH_OK) return rc;
    unsigned char *const d = (unsigned char *)lead->pm_batch.d;
    HIPCHK(lead, hipMemcpyAsync(d, img.data(), bytes, hipMemcpyHostToDevice, lead->stream));
    HIPCHK(lead, hipMemsetAsync(lead->d_resident, 0, CVH_RESIDENT_C1_BYTES, lead->stream));
    HIPCHK(lead, hipEventRecord(lead->ev0, lead->stream));
    for (size_t b = 0; b < launches.size(); ++b) {
      const PmBatchLaunch &bl = launches[b];
      const int np = (int)bl.members.size();
      size_t nmax = 0;
      for (int i : bl.members) nmax = ctxs[i]->n > nmax ? ctxs[i]->n : nmax;
      CvhPmBatchArgs ba;
      ba.planes = (const CvhPmBatchPlane *)(d + off[b].planes); ba.map = (const unsigned *)(d + off[b].map);
      ba.ntiles = bl.ntiles; ba.nplanes = np;
      HIPCHK(lead, cvh_launch_pm_load_batch((const CvhPmIoPlane *)(d + off[b].io_load), np, nmax, lead->stream));
      HIPCHK(lead, cvh_launch_pm_resident_batch(ba, bl.fast, bl.nr, lead->stream));
      HIPCHK(lead, cvh_launch_pm_store_batch((const CvhPmIoPlane *)(d + off[b].io_store), np, nmax, lead->stream));
    }
    HIPCHK(lead, hipEventRecord(lead->ev1, lead->stream));
    HIPCHK(lead, hipMemcpyAsync(lead->h_resident, lead->d_resident, 4, hipMemcpyDeviceToHost, lead->stream));
    HIPCHK(lead, hipStreamSynchronize(lead->stream));
    float ms = 0.f;
    HIPCHK(lead, hipEventElapsedTime(&ms, lead->ev0, lead->ev1));
    const bool gave_up = lead->h_resident[0] != 0;
    lead->h_resident[0] = 0;
    for (size_t b = 0; b < launches.size(); ++b) {
      const PmBatchLaunch &bl = launches[b];
      CvhLaunchNote nb{};
      CvhPmBatchArgs ba{};
      ba.ntiles = bl.ntiles;
      (void)cvh_launch_pm_resident_batch(ba, bl.fast, bl.nr, lead->stream, &nb);
      for (int i : bl.members) {
        cvh_context *c = ctxs[i];
        c->last_pm_ms = ms;
        planes_changed(c);
        c->pm_plane = gave_up ? -1 : 1;   // every launch of a member runs d_pm[0] -> d_pm[1]; the last round's is its last channel's
        if (bl.round != 0) continue;   // launch_info describes the launch of the member's first plane
        snprintf(c->pm_desc, sizeof(c->pm_desc), "kernel=%s grid=%u block=%u lds_bytes=%u steps_per_launch=%d tiles_y=%d tiles_x=%d launches=1 graph_launches=0 trips=%d planes=%d batch_planes=%d batch_launches=%d",
                 nb.name, nb.grid, nb.block, nb.lds, trips[i], (c->h + 8 * bl.nr - 1) / (8 * bl.nr), (c->w + cvh_resident_tile_w() - 1) / cvh_resident_tile_w(),
                 trips[i], c->C, (int)bl.members.size(), (int)launches.size());
      }
    }
    if (gave_up)
      return batch_fail(ctxs, n, CVH_ERR_HIP, "pm batch: a wait of the resident kernel gave up (a workgroup was not resident, or a fault); every member's planes are undefined");
  }
  // the members that are not fused: their own flow, as cvh_perona_malik
  for (int i = 0; i < n; ++i) {
    if (fused[i]) continue;
    rc = cvh_perona_malik(ctxs[i], K[i], L[i], T[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "pm batch: member %d: %s", i, ctxs[i]->err);
  }
  return CVH_OK;
}

