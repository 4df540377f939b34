// cvx_wave_body.inc -- the body of cvx_wave_kernel / cvx_wave_kernel_one (convex_kernels.hip), included into both, as geo_wave_body.inc
// is into the geodesic kernels and for its reason: C, FAST, STEP are the kernel's template arguments, `a` its record -- a record of the
// member table in the constant address space, or the by-value kernel argument itself --, TABLE and `parity` as set by the including kernel.
// TABLE: the member's workgroups lie behind a.first others and the set read is u[parity]; else the launch is the member's alone, reads
// u[0] and writes u[1] (the host swaps them per iteration).  !STEP: the start launch, which writes u[0] (parity is 0 there).
  constexpr int NS = cvh_cvx_nsums(C);
  if (STEP ? a.st->run.stopped : a.resume) return;   // (wave-uniform)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long item = (long long)(TABLE ? blockIdx.x - a.first : blockIdx.x) * (CVH_BLOCK / 64) + wave;
  if (item >= a.g.nitems) return;
  const int h = a.h, w = a.w;
  const MarchLane ml = march_lane(item, a.g.nwc, a.g.strip_rows, h, w);
  const int s0 = ml.s0, s1 = ml.s1, col = ml.col, colc = ml.colc;
  const bool lane_valid = ml.valid;
  const bool odd = TABLE && parity;
  const int si = odd ? 1 : 0;   // the set read; the other one is written
  double *const in_vbar = a.u[si].vbar, *const in_qx = a.u[si].qx, *const in_qy = a.u[si].qy;
  double *const out_vbar = a.u[si ^ 1].vbar, *const out_qx = a.u[si ^ 1].qx, *const out_qy = a.u[si ^ 1].qy;
  const gbytes_in plane[CVH_MAX_CHANNELS] = {(gbytes_in)a.img[0], (gbytes_in)a.img[1], (gbytes_in)a.img[2]};

  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;

  if (!STEP) {
    // v0 = the mask of the level set, vbar0 = v0, q = 0; the sums of v0 (exact integers) and no step: sum d^2 = 0
    const gdoubles_in u = (gdoubles_in)a.levelset;
    const gdoubles_out v = (gdoubles_out)a.v, vb = (gdoubles_out)in_vbar, qx = (gdoubles_out)in_qx, qy = (gdoubles_out)in_qy;
    for (int r = s0; r < s1; ++r) {
      const size_t o = (size_t)r * w + colc;
      const double v0 = (float)u[o] > 0.f ? 1.0 : 0.0;
      if (lane_valid) { v[o] = v0; vb[o] = v0; qx[o] = 0.0; qy[o] = 0.0; }
      acc[0] += v0;
#pragma unroll
      for (int k = 0; k < C; ++k) acc[1 + k] += (double)plane[k][o] * v0;
    }
  } else {
    const gdoubles_in ivb = (gdoubles_in)in_vbar, iqx = (gdoubles_in)in_qx, iqy = (gdoubles_in)in_qy;
    const gdoubles_out ovb = (gdoubles_out)out_vbar, oqx = (gdoubles_out)out_qx, oqy = (gdoubles_out)out_qy;
    const gdoubles_out v = (gdoubles_out)a.v;
    const gwords_in gq = (gwords_in)a.gq;   // (null: g = 1)
    const double tau = a.tau, sigma = a.sigma, mu = a.mu, nu = a.nu;
    double c1[C], c2[C], l1[C], l2[C];
#pragma unroll
    for (int k = 0; k < C; ++k) { c1[k] = a.st->c1[k]; c2[k] = a.st->c2[k]; l1[k] = a.lambda1[k]; l2[k] = a.lambda2[k]; }

    // every row and column is clamped to the plane: no load leaves the buffers
    auto vbar_at = [&](int r) -> double { return ivb[(size_t)clampi(r, 0, h - 1) * w + colc]; };
    auto rho_of = [&](size_t o) -> double { return mu * (gq ? (double)gq[o] * (1.0 / CVH_EDGE_ONE) : 1.0); };   // g = gq 2^-15, exact
    // rows g0 + 1 .. g0 + R of vbar and rows g0 .. g0 + R - 1 of v, qx, qy, the planes and the edge plane
    auto request = [&](int g0, double (&tb)[R], double (&tv)[R], double (&tx)[R], double (&ty)[R], int (&ti)[C][R], int (&tg)[R]) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        tb[j] = vbar_at(g0 + 1 + j);
        const size_t o = (size_t)clampi(g0 + j, 0, h - 1) * w + colc;
        // (halo lanes and lanes behind the last column read v at a column another lane or wave updates in place in this launch: harmless
        // only because their vn is neither stored -- lane_valid -- nor summed -- march_store_sum masks by ml.valid)
        tv[j] = v[o]; tx[j] = iqx[o]; ty[j] = iqy[o];
#pragma unroll
        for (int k = 0; k < C; ++k) ti[k][j] = plane[k][o];
        tg[j] = gq ? (int)gq[o] : CVH_EDGE_ONE;
      }
    };
    // the lane's column has a right neighbour / the row a lower one inside the plane: else the forward difference is 0
    const bool has_east = col < w - 1;

    double vb0 = vbar_at(s0);
    double nb[R], nv[R], nqx[R], nqy[R];
    int im[C][R], gm[R];
    request(s0, nb, nv, nqx, nqy, im, gm);
    // qy' of the row above the strip, from the OLD q and vbar of rows s0 - 1 and s0: the bits the strip above computes.  Row 0: 0
    double qyp = 0.0;
    if (s0 > 0) {
      const size_t o = (size_t)(s0 - 1) * w + colc;
      const double vbm = ivb[o];
      const double vbe = from_right_lane(vbm, vbm);
      const double dx = has_east ? vbe - vbm : 0.0;
      double px, py;
      cvx_dual<FAST>(iqx[o], iqy[o], dx, vb0 - vbm, sigma, rho_of(o), px, py);
      qyp = py;
    }

    for (int g0 = s0; g0 < s1; g0 += R) {
      double tb[R], tv[R], tx[R], ty[R];
      int ti[C][R], tg[R];
      const bool more = g0 + R < s1;   // (wave-uniform)
      if (more) request(g0 + R, tb, tv, tx, ty, ti, tg);
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int r = g0 + j;
        if (r < s1) {   // (wave-uniform: rows past the strip's end belong to the next strip)
          const double up = nb[j];
          double f[C];
#pragma unroll
          for (int k = 0; k < C; ++k) f[k] = (double)im[k][j];
          const double vbe = from_right_lane(vb0, vb0);   // (lane 63: its own, a column no lane of this wave uses)
          const double dx = has_east ? vbe - vb0 : 0.0;
          const double dy = r < h - 1 ? up - vb0 : 0.0;
          const double rho = mu * ((double)gm[j] * (1.0 / CVH_EDGE_ONE));
          double px, py;
          cvx_dual<FAST>(nqx[j], nqy[j], dx, dy, sigma, rho, px, py);
          const double pxl = from_left_lane(px, 0.0);
          const double div = (px - (col > 0 ? pxl : 0.0)) + (py - qyp);
          const double vo = nv[j];
          const double vn = cvx_primal<C, FAST>(f, c1, c2, l1, l2, nu, tau, div, vo);
          const double d = vn - vo;
          if (lane_valid) {
            const size_t o = (size_t)r * w + col;
            v[o] = vn; ovb[o] = (vn + vn) - vo; oqx[o] = px; oqy[o] = py;
          }
          acc[0] += vn;
#pragma unroll
          for (int k = 0; k < C; ++k) acc[1 + k] += f[k] * vn;
          acc[1 + C] += d * d;
          qyp = py; vb0 = up;
        }
      }
      if (more) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
          nb[j] = tb[j]; nv[j] = tv[j]; nqx[j] = tx[j]; nqy[j] = ty[j]; gm[j] = tg[j];
#pragma unroll
          for (int k = 0; k < C; ++k) im[k][j] = ti[k][j];
        }
      }
    }
  }
  double *row = a.partials + (size_t)item * NS;
#pragma unroll
  for (int s = 0; s < NS; ++s) march_store_sum(ml, acc[s], row + s);
