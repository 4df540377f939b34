// mp_wave_body.inc -- the body of mp_wave_kernel / mp_wave_kernel_one (multiphase_kernels.hip), included into both: C, FAST, STEP are the
// kernel's template arguments, `a` its record -- a record of the member table in the constant address space, or the by-value kernel
// argument itself --, TABLE and `parity` as set by the including kernel.  Text, not a function: the by-value kernel then compiles as
// the single call's kernel did before the batch existed (through a function taking the record by reference, the FAST three-channel
// step spilled 32 scalar registers where that kernel spills 12, and measured 2 % slower at 4096^2 x 3: DESIGN.md 4.17b).
// TABLE: the pair's workgroups lie behind a.first others and the buffers read are u[parity][.]; else the launch is the pair's alone,
// reads u[0][.] and writes u[1][.] (the host swaps them per iteration).
  constexpr int NS = cvh_mp_nsums(C);
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
  const gdoubles_in in1 = (gdoubles_in)(odd ? a.u[1][0] : a.u[0][0]), in2 = (gdoubles_in)(odd ? a.u[1][1] : a.u[0][1]);
  const gdoubles_out out1 = (gdoubles_out)(odd ? a.u[0][0] : a.u[1][0]), out2 = (gdoubles_out)(odd ? a.u[0][1] : a.u[1][1]);
  const gbytes_in plane[CVH_MAX_CHANNELS] = {(gbytes_in)a.img[0], (gbytes_in)a.img[1], (gbytes_in)a.img[2]};

  // the means this iteration uses and the parameters of the two equations: wave-uniform
  double c[4][C], l1[2][C], l2[2][C];
  if (STEP) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
#pragma unroll
      for (int ab = 0; ab < 4; ++ab) c[ab][k] = a.st->c[ab][k];
#pragma unroll
      for (int e = 0; e < 2; ++e) { l1[e][k] = a.lambda1[e][k]; l2[e][k] = a.lambda2[e][k]; }
    }
  }

  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;

  auto at = [&](gdoubles_in u, int r) -> double { return u[(size_t)clampi(r, 0, h - 1) * w + colc]; };
  // rows g0 + 1 .. g0 + R of both level sets and rows g0 .. g0 + R - 1 of the planes.  (A group of four rows ahead, where the localised
  // kernel asks for one: a row here is two doubles and C bytes, nothing enters or leaves a window)
  auto request = [&](int g0, double (&t1)[R], double (&t2)[R], int (&ti)[C][R]) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      t1[j] = at(in1, g0 + 1 + j);
      t2[j] = at(in2, g0 + 1 + j);
#pragma unroll
      for (int k = 0; k < C; ++k) ti[k][j] = plane[k][(size_t)clampi(g0 + j, 0, h - 1) * w + colc];
    }
  };

  double um1 = at(in1, s0 - 1), u01 = at(in1, s0), um2 = at(in2, s0 - 1), u02 = at(in2, s0);
  double nyp1 = 0.0, nyp2 = 0.0;
  double n1[R], n2[R];
  int im[C][R];
  request(s0, n1, n2, im);
  if (STEP) {
    nyp1 = ny_above<FAST>(s0, [&] { return at(in1, s0 - 2); }, um1, u01, n1[0]);
    nyp2 = ny_above<FAST>(s0, [&] { return at(in2, s0 - 2); }, um2, u02, n2[0]);
  }
  const double fx = (col <= 0) ? 0.0 : 1.0;
  auto curvature = [&](double um, double u0, double up, double &ny_prev) { return march_curvature<FAST>(um, u0, up, ny_prev, fx, col); };
  auto update = [&](double kappa, double F, double u0, int e) { return march_update<FAST>(kappa, F, u0, a.alpha[e], a.beta[e], a.gamma[e], eps, eps2, a.f.dk1); };

  for (int g0 = s0; g0 < s1; g0 += R) {
    double t1[R], t2[R];
    int ti[C][R];
    const bool more = g0 + R < s1;   // (wave-uniform)
    if (more) request(g0 + R, t1, t2, ti);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int r = g0 + j;
      if (r < s1) {   // (wave-uniform: rows past the strip's end belong to the next strip)
        const double up1 = n1[j], up2 = n2[j];
        double f[C];
#pragma unroll
        for (int k = 0; k < C; ++k) f[k] = (double)im[k][j];
        if (STEP) {
          const double h1 = heaviside<FAST>(u01, lane_valid, a.f, fc, satan), h2 = heaviside<FAST>(u02, lane_valid, a.f, fc, satan);
          const double k1 = curvature(um1, u01, up1, nyp1), k2 = curvature(um2, u02, up2, nyp2);
          double F1 = 0.0, F2 = 0.0;
#pragma unroll
          for (int k = 0; k < C; ++k) {
            const double q11 = (f[k] - c[0][k]) * (f[k] - c[0][k]), q10 = (f[k] - c[1][k]) * (f[k] - c[1][k]);
            const double q01 = (f[k] - c[2][k]) * (f[k] - c[2][k]), q00 = (f[k] - c[3][k]) * (f[k] - c[3][k]);
            F1 += h2 * (l2[0][k] * q01 - l1[0][k] * q11) + (1 - h2) * (l2[0][k] * q00 - l1[0][k] * q10);
            F2 += h1 * (l2[1][k] * q10 - l1[1][k] * q11) + (1 - h1) * (l2[1][k] * q00 - l1[1][k] * q01);
          }
          const double d1 = update(k1, F1, u01, 0), d2 = update(k2, F2, u02, 1);
          const double v1 = u01 + d1, v2 = u02 + d2;
          if (lane_valid) {
            const size_t o = (size_t)r * w + col;
            out1[o] = v1;
            out2[o] = v2;
          }
          add_pixel<C>(acc, heaviside<FAST>(v1, lane_valid, a.f, fc, satan), heaviside<FAST>(v2, lane_valid, a.f, fc, satan), f);
          acc[4 + 4 * C] += d1 * d1;
          acc[5 + 4 * C] += d2 * d2;
        } else {
          add_pixel<C>(acc, heaviside<FAST>(u01, lane_valid, a.f, fc, satan), heaviside<FAST>(u02, lane_valid, a.f, fc, satan), f);
        }
        um1 = u01; u01 = up1; um2 = u02; u02 = up2;
      }
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        n1[j] = t1[j]; n2[j] = t2[j];
#pragma unroll
        for (int k = 0; k < C; ++k) im[k][j] = ti[k][j];
      }
    }
  }
  double *row = a.partials + (size_t)item * NS;
#pragma unroll
  for (int s = 0; s < NS; ++s) march_store_sum(ml, acc[s], row + s);
