// geo_wave_body.inc -- the body of geo_wave_kernel / geo_wave_kernel_one (geodesic_kernels.hip), included into both, as mp_wave_body.inc
// is into the four-phase kernels and for its reason: C, FAST, STEP are the kernel's template arguments, `a` its record -- a record of the
// member table in the constant address space, or the by-value kernel argument itself --, TABLE and `parity` as set by the including kernel.
// TABLE: the member's workgroups lie behind a.first others and the buffer read is u[parity]; else the launch is the member's alone, reads
// u[0] and writes u[1] (the host swaps them per iteration).
  constexpr int NS = cvh_geo_nsums(C);
  __shared__ double satan[FAST ? CVH_ATAN2_N + 1 : 1];
  if (STEP && a.st->run.stopped) return;   // (uniform: before the barrier)
  if (FAST) stage_atan2(satan, a.f);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long item = (long long)(TABLE ? blockIdx.x - a.first : blockIdx.x) * (CVH_BLOCK / 64) + wave;
  if (item >= a.g.nitems) return;
  const int h = a.h, w = a.w;
  const MarchLane ml = march_lane(item, a.g.nwc, a.g.strip_rows, h, w);
  const int s0 = ml.s0, s1 = ml.s1, col = ml.col, colc = ml.colc;
  const bool lane_valid = ml.valid;
  const FarCoef fc = far_coef_of(a.f);
  const double eps = a.f.eps, eps2 = eps * eps;
  const bool odd = TABLE && parity;
  const gdoubles_in in = (gdoubles_in)(odd ? a.u[1] : a.u[0]);
  const gdoubles_out out = (gdoubles_out)(odd ? a.u[0] : a.u[1]);
  const gbytes_in plane[CVH_MAX_CHANNELS] = {(gbytes_in)a.img[0], (gbytes_in)a.img[1], (gbytes_in)a.img[2]};
  const gwords_in gq = (gwords_in)a.gq;

  // the means this iteration uses and the parameters: wave-uniform
  double c1[C], c2[C], l1[C], l2[C];
  if (STEP) {
#pragma unroll
    for (int k = 0; k < C; ++k) { c1[k] = a.st->c1[k]; c2[k] = a.st->c2[k]; l1[k] = a.lambda1[k]; l2[k] = a.lambda2[k]; }
  }

  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;

  // every row and column is clamped to the plane: no load leaves the buffers
  auto at = [&](int r) -> double { return in[(size_t)clampi(r, 0, h - 1) * w + colc]; };
  auto weight = [](int q) -> double { return (double)q * (1.0 / CVH_EDGE_ONE); };   // g = gq 2^-15, exact
  // rows g0 + 1 .. g0 + R of the level set and rows g0 .. g0 + R - 1 of the planes and of the edge plane (2 bytes beside the C bytes)
  auto request = [&](int g0, double (&t)[R], int (&ti)[C][R], int (&tg)[R]) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      t[j] = at(g0 + 1 + j);
      const size_t o = (size_t)clampi(g0 + j, 0, h - 1) * w + colc;
#pragma unroll
      for (int k = 0; k < C; ++k) ti[k][j] = plane[k][o];
      tg[j] = STEP ? (int)gq[o] : 0;
    }
  };

  double um = at(s0 - 1), u0 = at(s0);
  double gyp = 0.0;
  double n[R];
  int im[C][R], gm[R];
  request(s0, n, im, gm);
  if (STEP)
    gyp = gy_above<FAST>(s0, [&] { return at(s0 - 2); }, [&] { return weight((int)gq[(size_t)(s0 - 1) * w + colc]); }, um, u0, n[0], weight(gm[0]));
  const double fx = (col <= 0) ? 0.0 : 1.0;

  for (int g0 = s0; g0 < s1; g0 += R) {
    double t[R];
    int ti[C][R], tg[R];
    const bool more = g0 + R < s1;   // (wave-uniform)
    if (more) request(g0 + R, t, ti, tg);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int r = g0 + j;
      if (r < s1) {   // (wave-uniform: rows past the strip's end belong to the next strip)
        const double up = n[j];
        double f[C];
#pragma unroll
        for (int k = 0; k < C; ++k) f[k] = (double)im[k][j];
        double hv;
        if (STEP) {
          const double kappa = march_curvature_weighted<FAST>(um, u0, up, weight(gm[j]), gyp, fx, col);
          double F = 0.0;
#pragma unroll
          for (int k = 0; k < C; ++k) F += l2[k] * ((f[k] - c2[k]) * (f[k] - c2[k])) - l1[k] * ((f[k] - c1[k]) * (f[k] - c1[k]));
          const double d = march_update<FAST>(kappa, F, u0, a.alpha, a.beta, a.gamma, eps, eps2, a.f.dk1);
          const double v = u0 + d;
          if (lane_valid) out[(size_t)r * w + col] = v;
          hv = heaviside<FAST>(v, lane_valid, a.f, fc, satan);
          acc[1 + C] += d * d;
        } else {
          hv = heaviside<FAST>(u0, lane_valid, a.f, fc, satan);
        }
        acc[0] += hv;
#pragma unroll
        for (int k = 0; k < C; ++k) acc[1 + k] += f[k] * hv;
        um = u0; u0 = up;
      }
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        n[j] = t[j]; gm[j] = tg[j];
#pragma unroll
        for (int k = 0; k < C; ++k) im[k][j] = ti[k][j];
      }
    }
  }
  double *row = a.partials + (size_t)item * NS;
#pragma unroll
  for (int s = 0; s < NS; ++s) march_store_sum(ml, acc[s], row + s);
