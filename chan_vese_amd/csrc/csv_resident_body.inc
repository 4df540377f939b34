// csv_resident_body.inc — the body of csv_resident_kernel<NRT> (one channel) and csv_resident_kernel<3, NRT> (csv_resident_kernel.hip), included inside
// both.  Expects `a` (const CvhStepArgs, the launch arguments), C (channels: 1 or 3) and NRT (rows per wave of a straight-line flavour, or 0) in scope.
  static_assert(C == 1 || C == 3, "one or three channels");
  static_assert(NRT * RT_WAVES <= rt_hmax(C), "a straight-line flavour's tile must fit");
  using L = ResSmem<C>;
  constexpr int NS = L::NS, NP = L::NP;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *su = smem + L::off_u;
  unsigned char *simg = reinterpret_cast<unsigned char *>(smem + L::off_img);
  double *slut = smem + L::off_lut;
  double *satan = smem + L::off_atan;
  double *snxl = smem + L::off_nxl;
  double *sred = smem + L::off_red;
  double *s_bc = smem + L::off_flag;      // 1 + 2C doubles of broadcast scratch (+ 1)
  int *s_flag = (int *)(s_bc + L::NBC);
  int *s_mflag = s_flag + 12;             // master workgroup: generation each wave's share of the arrivals is complete for
  constexpr unsigned kLutAddr = (unsigned)(L::off_lut * sizeof(double));   // LDS byte address of the region-term table (the dynamic block starts at 0)
  if (!lds_base_is_zero(smem)) __builtin_trap();                          // (folds away: no static LDS in this kernel)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < RT_WAVES) s_mflag[tid] = 0;
  if (tid == 0) s_flag[9] = 0;             // master workgroup: waves whose border stores are acknowledged, counted over the launch
  const int h = a.h, w = a.w;
  CvhResident *const rs = a.resident;
  // sticky stop flag of an EARLIER launch (src/main.cpp:1000): read at agent scope -- every workgroup must see the same value, and a
  // cooperative launch is dispatched through its own queue (a cached copy of the word is not to be trusted here)
  if (tid == 0) s_flag[0] = __hip_atomic_load(&a.st->stopped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const int stopped_before = s_flag[0];
  __syncthreads();
  if (stopped_before != 0) return;
  // index of this launch's first iteration inside the run: a launch ARGUMENT (the host's count of the iterations it has enqueued since
  // the run counter was reset), not read from the state block: a stale cached copy of that word would shift every trace row
  const int t_first = a.res_t0;

  // ---- this workgroup's tile
  const int tr = a.tiles_y, tc = a.tiles_x, ntiles = tr * tc;
  const int bid = (int)blockIdx.x;
  const int ty = bid / tc, tx = bid % tc;
  const int r0 = (int)(((long)h * ty) / tr), r1 = (int)(((long)h * (ty + 1)) / tr);
  const int TH = r1 - r0;                              // <= rt_hmax(C) (host)
  const int c0 = tx * RT_W;
  const int TWv = (w - c0) < RT_W ? (w - c0) : RT_W;   // even (host: w even)
  // LDS address of tile element (row r in -2 .. TH, column c in -2 .. 129)
  auto S = [&](int r, int c) -> double * { return su + (r + 2) * RT_PITCH + (c + 2); };

  // ---- once per launch: tables, image tile, level-set tile with its halo ring straight from the plane (clamped = BORDER_REPLICATE)
  for (int q = tid; q < CVH_ATAN2_N; q += RT_THREADS) satan[q] = a.atan2_tab[q];
  if ((w & 15) == 0) {                                                   // rows are 16-byte aligned and the tile's width is a multiple of 16
    for (int q = tid; q < TH * (RT_W / 16); q += RT_THREADS) {           // 16-byte pieces of the image tile
      const int r = q / (RT_W / 16), p = q % (RT_W / 16);
      const int col = c0 + 16 * p < w ? c0 + 16 * p : w - 16;            // pieces beyond the image: no lane reads them
      const uint4 v = *reinterpret_cast<const uint4 *>(a.img[0] + (size_t)(r0 + r) * w + col);
      *reinterpret_cast<uint4 *>(simg + r * RT_W + 16 * p) = v;
      if (C > 1) {
#pragma unroll
        for (int ch = 1; ch < C; ++ch)
          *reinterpret_cast<uint4 *>(simg + ch * L::img_bytes + r * RT_W + 16 * p) = *reinterpret_cast<const uint4 *>(a.img[ch] + (size_t)(r0 + r) * w + col);
      }
    }
  } else {
    for (int q = tid; q < TH * RT_W; q += RT_THREADS) {                  // other widths: byte by byte (once per launch)
      const int r = q / RT_W, c = q % RT_W;
      simg[q] = a.img[0][(size_t)(r0 + r) * w + clampi(c0 + c, 0, w - 1)];
      if (C > 1) {
#pragma unroll
        for (int ch = 1; ch < C; ++ch) simg[ch * L::img_bytes + q] = a.img[ch][(size_t)(r0 + r) * w + clampi(c0 + c, 0, w - 1)];
      }
    }
  }
  for (int q = tid; q < (TH + 3) * RT_PITCH; q += RT_THREADS) {
    const int r = q / RT_PITCH - 2, c = q % RT_PITCH - 2;
    const int gr = clampi(r0 + r, 0, h - 1), gc = clampi(c0 + c, 0, w - 1);
    su[q] = a.u_in[(size_t)gr * w + gc];
  }
  // Sum sets (chain_device.h): the launch reads set p0 (the sums of the level set it starts from) and leaves set p0 + executed filled and
  // set p0 + executed + 1 clear -- the per-launch invariant -- when it ends.  In between the sums do not touch the sets: every tile hands
  // its fixed-point integers to the master with its arrival line, and the master adds them (integer addition: exact, order-free, the
  // very totals the per-launch path's atomic adds produce).
  // region means of the level set the launch starts from (later iterations get theirs with the release)
  double cm1[C], cm2[C];
  double &c1 = cm1[0], &c2 = cm2[0];        // (one channel's names)
  {
    const long long entry = a.chain->v[a.chain_phase & 3][lane];
    chain_means<C>(a, entry, cm1, cm2);
    if (t_first > 0) {   // continuing on a level set an earlier iteration left with a NaN (its norm says so): NaN means, as below
      const double last = a.st->norm;
      if (last != last) {
#pragma unroll
        for (int k = 0; k < C; ++k) cm1[k] = cm2[k] = last;
      }
    }
  }
  __syncthreads();

  const double l1 = a.lambda1[0], l2 = a.lambda2[0];
  const double eps = a.eps, eps2 = eps * eps;
  const FarCoef fc = {a.far_k[0], a.far_k[1], a.far_k[2], a.far_k[3], a.far_k[4], a.far_thr};
  // this wave's band of tile rows
  const int rb0 = NRT ? NRT * wave : (TH * wave) / RT_WAVES, rb1 = NRT ? rb0 + NRT : (TH * (wave + 1)) / RT_WAVES;
  const int ca = 2 * lane;                                  // tile column of pixel a
  const bool lane_valid = ca < TWv;
  const double fxa = (c0 + ca <= 0) ? 0.0 : 1.0;            // kappa_x(i, 0) = 0 (src/main.cpp:371)
  double *const halo_mine[2] = {a.res_halo + (size_t)bid * RT_HALO, a.res_halo + ((size_t)ntiles + bid) * RT_HALO};
  auto norm = [&](double fwd, double bwd, double c) -> double { return normalised4(fwd, bwd, c + c); };

  // diagnostic stamps (option "debug_times", tools/resident_timeline.py): 12 words per workgroup, taken around iteration kStampIt
  constexpr int kStampIt = 3;
  auto stamp = [&](int it_now, int it_want, int slot) {
    if (a.dbg_times && it_now == it_want && tid == 0) a.dbg_times[(size_t)bid * 12 + slot] = __builtin_amdgcn_s_memrealtime();
  };
  int executed = 0;
  bool gave_up = false;
  const int nit = a.res_steps;
  int it = 0;
  // The master's books of one iteration (thread 0 of workgroup 0): trace row, state block and -- when the launch ends or the stop rule
  // fired -- the two words the host polls in pinned memory.  (Inside a launch the host does not need them: it runs at most four launches
  // ahead of the count the LAST word of a launch reports; a store to host memory is acknowledged after 1.5 us, and a wave cannot wait for
  // anything else of its own without waiting for that.)
  auto book = [&](const double (&m1)[C], const double (&m2)[C], double nrm, int stop_now, bool last) {
    if (tid != 0) return;
    CvhState *st = a.st;
    const int t = t_first + it;
    constexpr int TR = 2 * C + 1;          // a trace row: c1_0 .. c1_{C-1}, c2_0 .. c2_{C-1}, norm (the per-launch flow's order)
    if (a.trace && t < a.trace_cap) {
#pragma unroll
      for (int k = 0; k < C; ++k) { a.trace[(size_t)t * TR + k] = m1[k]; a.trace[(size_t)t * TR + C + k] = m2[k]; }
      a.trace[(size_t)t * TR + 2 * C] = nrm;
    }
    st->norm = nrm;
    st->steps_done = t + 1;
    st->pending = 0;
    if (stop_now) st->stopped = 1;
    if (a.host_status && last) {
      __hip_atomic_store(&a.host_status[1], stop_now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&a.host_status[0], t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  };
  // (master workgroup: the release it wrote itself, handed from thread 0 to the workgroup without a poll)
  OwnRelease<C> own = {-1, 0, {}, {}};
  bool book_pending = false;   // (wave 0 of the master) iteration `it` is released but not yet booked
  double book_nrm = 0.0;
  bool have_go = false;      // (workgroup-uniform) the release into the next iteration was handed over inside the workgroup
  int go_known = -1;
  if (bid == 0 && tid == 0) { rs->pad[0] = (unsigned)t_first; rs->pad[1] = (unsigned)nit; rs->pad[2] = (unsigned)a.st->steps_done; }   // (diagnostic record of the launch)
  // ---- what an iteration reads before any wave writes and that does not wait for the release (c1 / c2): every wave takes the rows around
  // its band into registers, one thread per row computes the normalised x-gradient of tile column -1 (nobody owns that column; lane 0 needs
  // it for column 0), and ny of the row above the band.  Called when the tile and its halo ring are complete: before the loop, and at the end
  // of an iteration behind the fetch of the neighbours' borders -- off the path from the release into the march.
  double2_t p_um = {0.0, 0.0}, p_u0 = {0.0, 0.0}, p_ubot = {0.0, 0.0};
  double p_uw = 0.0, p_ue = 0.0, p_nypa = 0.0, p_nypb = 0.0;
  auto pre_reads = [&]() {
    if (tid >= 256 && tid - 256 < TH) snxl[tid - 256] = norm(*S(tid - 256, 0), *S(tid - 256, -2), *S(tid - 256, -1));
    const double2_t um2_0 = *reinterpret_cast<const double2_t *>(S(rb0 - 2, ca));
    p_um = *reinterpret_cast<const double2_t *>(S(rb0 - 1, ca));
    p_u0 = *reinterpret_cast<const double2_t *>(S(rb0, ca));
    p_ubot = *reinterpret_cast<const double2_t *>(S(rb1, ca));
    p_uw = *S(rb0, ca - 1); p_ue = *S(rb0, ca + 2);
    const double2_t u1st = *reinterpret_cast<const double2_t *>(S(rb0 + 1 < rb1 ? rb0 + 1 : rb0, ca));   // row rb0 + 1 (own band, if it has one)
    if (rb1 > rb0) {
      p_nypa = norm(p_u0.x, um2_0.x, p_um.x); p_nypb = norm(p_u0.y, um2_0.y, p_um.y);   // ny at row rb0 - 1
      if (r0 + rb0 == 0) {   // kappa_y(0, .) = 0 (:372): ny_prev := row 0's own ny, the very expression the row uses
        const double2_t up0 = (rb0 + 1 < rb1) ? u1st : p_ubot;
        p_nypa = norm(up0.x, p_um.x, p_u0.x); p_nypb = norm(up0.y, p_um.y, p_u0.y);
      }
    }
  };
  for (it = 0; it < nit; ++it) {
    const int phase = (a.chain_phase + it) & 3;
    // ---- the release behind iteration it - 1: leave bit and the region means of u(it); the halos were fetched while waiting
    if (it > 0) {
      const int go = have_go ? go_known : wg_wait_go<C>(rs, bid, it, a, s_bc, cm1, cm2, own);   // (have_go: the master workgroup, short way)
      have_go = false;
      if (go < 0) { gave_up = true; break; }
      if (go & 1) break;
    }
    stamp(it, kStampIt, 0); stamp(it, kStampIt + 1, 8);       // released into this iteration
    // ---- table of the variance term (:307-310, :979, :985)
    if (C == 1) {
      if (tid < 256) {
        const double v = (double)tid;
        const double d1 = v - c1, d2 = v - c2;
        const double reg = (d2 * d2) * l2 - (d1 * d1) * l1;
        slut[2 * tid] = __builtin_fma(reg, a.beta, a.gamma);
        slut[2 * tid + 1] = v;
      }
    } else if (tid < 256) {                  // one table per channel, as csv_wave2_kernel<3, ...> fills them: -nu dt rides in channel 0's
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const double v = (double)tid;
        const double d1 = v - cm1[k], d2 = v - cm2[k];
        const double reg = (d2 * d2) * a.lambda2[k] - (d1 * d1) * a.lambda1[k];
        slut[2 * (k * 256 + tid)] = (k == 0) ? __builtin_fma(reg, a.beta, a.gamma) : reg * a.beta;
        slut[2 * (k * 256 + tid) + 1] = v;
      }
    }
    // (what an iteration needs that does NOT depend on the region means -- column -1's normalised x-gradient, the rows around the band in
    // registers, ny of the row above the band -- was taken BEFORE the release was waited for: pre_reads, at the end of the previous iteration)
    if (it == 0) pre_reads();
    double2_t um = p_um, u0 = p_u0;
    const double2_t ubot = p_ubot;
    double uw = p_uw, ue = p_ue;
    lds_barrier();                                             // (LDS only: the master's bookkeeping stores may still be in flight)
    stamp(it, kStampIt, 1);                                    // table in LDS, band borders in registers

    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0;
    if (rb1 > rb0) {
      double nypa = p_nypa, nypb = p_nypb;                      // ny at row rb0 - 1 (pre_reads)
      auto pixel = [&](double c, double n_, double s_, double nx, double nxl, double fx, double &nyp, int byte, double &ud_out,
                       double &Ik_out) -> double {
        const double ny = norm(s_, n_, c);
        const double kappa = __builtin_fma(nx - nxl, fx, ny - nyp);
        const double2_t e = lds_read_d2(kLutAddr + (unsigned)byte);      // `byte`: the entry's byte offset (sample x 16)
        double ud = __builtin_fma(kappa, a.alpha, e.x);                  // :985
        ud = ud * rcp_refined(inv_delta_eps(c, eps2, a.dk1));            // :992
        nyp = ny;
        ud_out = ud; Ik_out = e.y;
        return c + ud;                                                   // :994
      };
      // three channels: the same update with the region term summed over the channels' tables (csv_wave2_kernel.hip, pixel3)
      auto pixel3 = [&](double c, double n_, double s_, double nx, double nxl, double fx, double &nyp, const int (&byte)[C], double &ud_out,
                        double (&Ik)[C]) -> double {
        const double ny = norm(s_, n_, c);
        const double kappa = __builtin_fma(nx - nxl, fx, ny - nyp);
        double reg;
        {
          const double2_t e0 = lds_read_d2(kLutAddr + (unsigned)byte[0]);
          reg = e0.x; Ik[0] = e0.y;
#pragma unroll
          for (int ch = 1; ch < C; ++ch) {
            const double2_t e = lds_read_d2(kLutAddr + (unsigned)(ch * 4096) + (unsigned)byte[ch]);
            reg += e.x; Ik[ch] = e.y;
          }
        }
        double ud = __builtin_fma(kappa, a.alpha, reg);                  // :985
        const double qd = __builtin_fma(c, c, eps2) * a.dk1;             // 1/delta_eps(u)
        const double q0 = __builtin_amdgcn_rcp(qd);
        const double er = __builtin_fma(-qd, q0, 1.0);
        ud = ud * __builtin_fma(__builtin_fma(er, er, er), q0, q0);      // :992
        nyp = ny;
        ud_out = ud;
        return c + ud;                                                   // :994
      };
      // One row: everything up to the new values and the far-field form of H - 1/2 on every lane (branch-free); the lanes near
      // the contour are corrected per group of four rows (csv_wave2_kernel.hip, DEFER)
      double2_t keep[4];
      int smp_keep[4];
      int rel_keep[4];                       // three channels: the row inside the band (its samples stay in the LDS image tiles)
      unsigned long long near_mask[4];       // lanes below the far-field threshold, per row of the current group (csv_wave2_kernel.hip: four independent masks are the fastest form)
      // (no branch inside a row: a group of four rows is one basic block and hipcc overlaps the rows' dependent chains)
      // (rel = row inside the band: a constant in the straight-line flavours, where every address below is base + immediate)
      double *const pb = S(rb0, ca);
      const unsigned char *const simg_b = simg + rb0 * RT_W + ca;
      const double *const snxl_b = snxl + rb0;
      // Which form of H_eps a BAND takes this iteration is decided per wave from its first row (csv_wave2_kernel.hip, near_strip): where
      // most of that row is below the far-field threshold the wave runs the copy of the march that takes the table form of every
      // pixel behind the rows of a group (valid for any u, nothing to correct) -- one form per pixel instead of three.
      const bool near_band = a.near_switch &&
          __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane_valid && (fabs(u0.x) < fc.thr || fabs(u0.y) < fc.thr))) >= 32;
      auto row = [&](int rel, int k, auto near_tag) {
        constexpr bool NEARFORM = decltype(near_tag)::value;
        const bool lastrow = rel + 1 >= (NRT ? NRT : rb1 - rb0);     // wave-uniform; a constant in the straight-line flavours
        double2_t up;
        double uw_n = 0.0, ue_n = 0.0;
        // below the band's last row: the copy taken before the march -- the band below may have rewritten its first row already
        if (NRT) {
          if (lastrow) up = ubot;
          else { up = *reinterpret_cast<const double2_t *>(pb + (rel + 1) * RT_PITCH); uw_n = pb[(rel + 1) * RT_PITCH - 1]; ue_n = pb[(rel + 1) * RT_PITCH + 2]; }
        } else {
          const double2_t up_l = *reinterpret_cast<const double2_t *>(pb + (rel + 1) * RT_PITCH);
          uw_n = pb[(rel + 1) * RT_PITCH - 1]; ue_n = pb[(rel + 1) * RT_PITCH + 2];   // (unused behind the band's last row)
          up = double2_t{lastrow ? ubot.x : up_l.x, lastrow ? ubot.y : up_l.y};
        }
        const int smp = (int)*reinterpret_cast<const unsigned short *>(simg_b + rel * RT_W);
        const int ba = (int)byte_x16<0>((unsigned)smp), bb = (int)byte_x16<1>((unsigned)smp);   // sample x 16 in one SDWA instruction each (wave_math.h)
        int sa[C], sb[C];                                            // three channels: the entries' byte offsets per channel
        sa[0] = ba; sb[0] = bb;
#pragma unroll
        for (int ch = 1; ch < C; ++ch) {
          const unsigned sc = (unsigned)*reinterpret_cast<const unsigned short *>(simg_b + ch * L::img_bytes + rel * RT_W);
          sa[ch] = (int)byte_x16<0>(sc); sb[ch] = (int)byte_x16<1>(sc);
        }
        const double nxl0 = snxl_b[rel];
        // x-gradients first: nx(b) is the west gradient of lane + 1's a (DPP), nx(a) the west gradient of b
        const double nxa = norm(u0.y, uw, u0.x);
        const double nxb = norm(ue, u0.x, u0.y);
        const double nxla = dpp_from_left_or(nxl0, nxb);          // lane 0 has no lane to its left: it keeps the pre-pass's value
        double uda, udb, Ia, Ib;
        double Ika[C], Ikb[C];
        double va, vb;
        if (C == 1) {
          va = pixel(u0.x, um.x, up.x, nxa, nxla, fxa, nypa, ba, uda, Ia);
          vb = pixel(u0.y, um.y, up.y, nxb, nxa, 1.0, nypb, bb, udb, Ib);
        } else {
          va = pixel3(u0.x, um.x, up.x, nxa, nxla, fxa, nypa, sa, uda, Ika);
          vb = pixel3(u0.y, um.y, up.y, nxb, nxa, 1.0, nypb, sb, udb, Ikb);
        }
        keep[k] = double2_t{va, vb};
        smp_keep[k] = smp;
        rel_keep[k] = rel;
        // in place: every reader of the old row i has it in registers.  Lanes beyond a ragged tile's width write cells nobody owns
        // (the halo column among them: it was read a row ahead and is refreshed before the next iteration)
        *reinterpret_cast<double2_t *>(pb + rel * RT_PITCH) = keep[k];
        if (!NEARFORM) {
          const double hva = heaviside_centred_far(va, fc), hvb = heaviside_centred_far(vb, fc);
          near_mask[k] = __builtin_amdgcn_ballot_w64(fabs(va) < fc.thr || fabs(vb) < fc.thr);
          acc[0] += hva; acc[0] += hvb;
          if (C == 1) { acc[2] = __builtin_fma(Ia, hva, acc[2]); acc[2] = __builtin_fma(Ib, hvb, acc[2]); }
          else {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) { acc[2 + ch] = __builtin_fma(Ika[ch], hva, acc[2 + ch]); acc[2 + ch] = __builtin_fma(Ikb[ch], hvb, acc[2 + ch]); }
          }
        }
        acc[2 + 2 * C] = __builtin_fma(uda, uda, acc[2 + 2 * C]); acc[2 + 2 * C] = __builtin_fma(udb, udb, acc[2 + 2 * C]);
        um = u0; u0 = up; uw = uw_n; ue = ue_n;
      };
      auto correct = [&](int k, auto near_tag) {
        constexpr bool NEARFORM = decltype(near_tag)::value;
        if (NEARFORM || near_mask[k] != 0ull) {
          const double xa = keep[k].x, xb = keep[k].y;
          double da, db;
          if (NEARFORM) {   // the rows added nothing for H
            da = heaviside_centred_near(xa, a.inv_eps, satan); db = heaviside_centred_near(xb, a.inv_eps, satan);
          } else {
            da = near_field_correction(xa, a.inv_eps, satan, fc);
            db = near_field_correction(xb, a.inv_eps, satan, fc);
          }
          acc[0] += da; acc[0] += db;
          acc[2] = __builtin_fma((double)(smp_keep[k] & 0xff), da, acc[2]);
          acc[2] = __builtin_fma((double)(smp_keep[k] >> 8), db, acc[2]);
#pragma unroll
          for (int ch = 1; ch < C; ++ch) {
            const int sc = (int)*reinterpret_cast<const unsigned short *>(simg_b + ch * L::img_bytes + rel_keep[k] * RT_W);
            acc[2 + ch] = __builtin_fma((double)(sc & 0xff), da, acc[2 + ch]);
            acc[2 + ch] = __builtin_fma((double)(sc >> 8), db, acc[2 + ch]);
          }
        }
      };
      // Two waves share a SIMD and at equal priority the arbiter serves the OLDER one first: it is through its band after 7.3 us, the younger
      // then runs alone -- a single wave hides no latency -- until 12 us (profiles/r03_C4/resident_timeline_2048.txt).  A wave lowers its priority
      // with every quarter of its band (as the per-launch kernels do by quarters of their strips): whoever is AHEAD yields, the two leapfrog by
      // groups of rows and finish together, two waves overlapping to the end.  (option "res_prio", default on)
      auto quarter_prio = [&](int done, int of) {
        if (!a.res_prio) return;
        const int q = of >= 4 ? (4 * done) / of : done;      // quarters of the band behind this wave
        if (q <= 0) __builtin_amdgcn_s_setprio(3);
        else if (q == 1) __builtin_amdgcn_s_setprio(2);
        else if (q == 2) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      };
      auto march = [&](auto near_tag) {
        constexpr bool NEARFORM = decltype(near_tag)::value;
        if (NRT >= 16 && NEARFORM) {
          // (the near copy of a 16-row band is a LOOP over its four groups: unrolled, the table forms of sixteen rows in flight took the
          // kernel to 256 VGPRs and 141 spilled registers, and values that live across the march were reloaded from scratch on the
          // far path as well)
#pragma unroll 1
          for (int g = 0; g < NRT / 4; ++g) {
            quarter_prio(4 * g, NRT);
#pragma unroll
            for (int k = 0; k < 4; ++k) row(4 * g + k, k, near_tag);
#pragma unroll
            for (int k = 0; k < 4; ++k) correct(k, near_tag);
          }
        } else if (NRT >= 4) {
#pragma unroll
          for (int g = 0; g < NRT / 4; ++g) {
            quarter_prio(4 * g, NRT);
#pragma unroll
            for (int k = 0; k < 4; ++k) row(4 * g + k, k, near_tag);
            if (NEARFORM || (near_mask[0] | near_mask[1] | near_mask[2] | near_mask[3]) != 0ull) {
#pragma unroll
              for (int k = 0; k < 4; ++k) correct(k, near_tag);
            }
          }
        } else if (NRT == 2) {
          row(0, 0, near_tag); correct(0, near_tag);
          row(1, 0, near_tag); correct(0, near_tag);
        } else {
          int rel = 0;
          for (; rel + 4 <= rb1 - rb0; rel += 4) {
            quarter_prio(rel, rb1 - rb0);
#pragma unroll
            for (int k = 0; k < 4; ++k) row(rel + k, k, near_tag);
            if (NEARFORM || (near_mask[0] | near_mask[1] | near_mask[2] | near_mask[3]) != 0ull) {
#pragma unroll
              for (int k = 0; k < 4; ++k) correct(k, near_tag);
            }
          }
          for (; rel < rb1 - rb0; ++rel) { row(rel, 0, near_tag); correct(0, near_tag); }
        }
      };
      if (near_band) march(std::true_type{}); else march(std::false_type{});
      if (a.res_prio) __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = lane_valid ? acc[s] : 0.0;   // lanes beyond the image contribute nothing
    }
    stamp(it, kStampIt, 2);                                    // (thread 0's wave) march done
    if (a.dbg_times && it == kStampIt && lane == 0 && (bid == 0 || bid == 100 || bid == 255))   // diagnostic: every wave of three tiles
      a.dbg_times[(size_t)CVH_RESIDENT_MAX_TILES * 12 + 16 + (bid == 0 ? 0 : bid == 100 ? 8 : 16) + wave] = __builtin_amdgcn_s_memrealtime();
    // ---- the tile's sums and its arrival.  One channel, H' sums: of the NS sums only [0] sum H', [2] sum I H' and [4] sum u_diff^2 are
    // carried.  Every wave reduces its three (DPP), lane 0 leaves them in LDS, ONE barrier (it also orders the tile writes before the border
    // reads below), and the three threads that store the arrival add the eight partials in a fixed order -- nobody else needs the totals.
    // (sred[0 .. 24): these partials; sred[24 .. 36): the master's, below)
    {
      const double v0 = wave_sum(acc[0]), v2 = wave_sum(acc[2]), v4 = wave_sum(acc[2 + 2 * C]);
      if (lane == 0) { sred[wave * NP] = v4; sred[wave * NP + 1] = v0; sred[wave * NP + 2] = v2; }
#pragma unroll
      for (int ch = 1; ch < C; ++ch) {       // three channels: NP = 5 sums per wave, sum I_1 H' and sum I_2 H' behind the three
        const double vk = wave_sum(acc[2 + ch]);
        if (lane == 0) sred[wave * NP + 2 + ch] = vk;
      }
    }
    __syncthreads();
    stamp(it, kStampIt, 3);                                    // all waves done, sums in LDS
    executed = it + 1;
    const unsigned gen = (unsigned)(it + 1);
    // three 16-byte lines {generation, payload}: sum u_diff^2, and the fixed-point sums the next iteration's means come from (distinct
    // addresses: 256 arrivals on one counter serialise for 6 us).  The arrival does not wait for the border stores below: the master needs
    // the sums only, the neighbours get their own signal.  (Two pieces -- the 64-bit sum of H' split over the spare words -- were tried: a third
    // fewer arrival stores and polls, and no faster: 13.03 vs 12.92 us at 2048^2, 5.73 vs 5.39 at 512^2, gpurun_out/r4s50.)
    // (three channels: five pieces -- sum I_k H' with its own scale chain_scale[1 + k]; the fifth lives in flag_c3, behind what one channel addresses)
    if (tid < NP) {
      double t = sred[tid];
#pragma unroll
      for (int wv = 1; wv < RT_WAVES; ++wv) t += sred[wv * NP + tid];   // fixed order
      const unsigned long long payload = tid == 0 ? (unsigned long long)__double_as_longlong(t)
                                       : (unsigned long long)__double2ll_rn(t * a.chain_scale[tid - 1]);
      if (C == 1 || tid < 4)
        st_line16_u64(rs->flag, ((unsigned)tid * CVH_RESIDENT_MAX_TILES + (unsigned)bid) * 16u, gen, 0u, payload);   // piece-major: the master's polls read neighbouring entries
      else st_line16_u64(rs->flag_c3, (unsigned)bid * 16u, gen, 0u, payload);
    }
    // ---- what crosses to the neighbours: the tile's border (6 x 128 doubles, agent-scope stores) and, once those are acknowledged, the
    // border signal; then the neighbours' borders of u(it + 1) -- they exist as soon as the up-to-four neighbours have stored THEIR signal --
    // go into the halo ring while the barrier completes; at the image's border: BORDER_REPLICATE from the tile's own edge (src/main.cpp:351-354)
    double *const hb = halo_mine[it & 1];
    auto border_value = [&](int q) -> double {
      const int piece = q / RT_W, k = q % RT_W;
      if (piece < 2) return *S(TH - 2 + piece, k);                    // bottom two rows   (TH >= 2: host)
      if (piece == 2) return *S(0, k);                                // top row
      if (piece < 5) return *S(k < TH ? k : 0, TWv - 5 + piece);      // right two columns: TWv - 2, TWv - 1
      return *S(k < TH ? k : 0, 0);                                   // left column
    };
    // two neighbouring elements of a piece with ONE 16-byte store (RT_W is even: a pair never straddles two pieces): 384 stores per tile
    auto store_border = [&](int p) {
      const double v0 = border_value(2 * p), v1 = border_value(2 * p + 1);
      const unsigned long long b0 = (unsigned long long)__double_as_longlong(v0), b1 = (unsigned long long)__double_as_longlong(v1);
      __builtin_amdgcn_raw_buffer_store_b128(u32x4r_t{(unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1, (unsigned)(b1 >> 32)}, make_rsrc(hb, 0x7fffffffu),
                                             (unsigned)p * 16u, 0u, 16 /* sc1 */);
    };
    constexpr int kPairs = 3 * RT_W;
    const bool want_borders = it + 1 < nit;
    const int nb_lane = lane == 0 ? (ty > 0 ? bid - tc : -1) : lane == 1 ? (ty < tr - 1 ? bid + tc : -1) : lane == 2 ? (tx > 0 ? bid - 1 : -1)
                        : lane == 3 ? (tx < tc - 1 ? bid + 1 : -1) : -1;          // lanes 0-3 of a polling wave watch one neighbour each
    auto tagged = [&](const u32x4r_t &f) -> bool { return f.x >= gen && f.x != 0xffffffffu; };
    // (a wave-wide bounded wait for the lanes' neighbours)
    auto neighbours_arrived = [&]() -> int {
      bool sat = nb_lane < 0;
      for (int i = 0; i < a.res_poll_cap; ++i) {
        if (!sat) sat = tagged(ld_line16(rs->hflag, (unsigned)(nb_lane < 0 ? 0 : nb_lane) * 64u));
        if (__builtin_amdgcn_ballot_w64(!sat) == 0ull) return 1;
        if ((i & 15) == 15 && ld_agent((const unsigned *)&rs->error) != 0u) break;
        __builtin_amdgcn_s_sleep(2);
      }
      return 0;
    };
    const double *const hbn = a.res_halo + (size_t)(it & 1) * ntiles * RT_HALO;
    // element q of the 6 x 128 border: its value (a neighbour's store, or the tile's own edge) into the halo cell it belongs to
    // pair p of the 6 x 128 border (elements 2p, 2p + 1 of one piece): the values (a neighbour's 16-byte store, or the tile's own edge) into
    // the two halo cells they belong to
    auto fetch = [&](int p) {
      const int q = 2 * p, piece = q / RT_W, k = q % RT_W;
      double *d0, *d1;
      int nb;              // the neighbour the piece comes from (-1: the image ends here)
      double e0, e1;       // ... and then: the tile's own edge
      if (piece < 2) {            // top halo rows -2, -1 <- the tile above's bottom two rows
        d0 = S(piece - 2, k); d1 = S(piece - 2, k + 1);
        nb = ty > 0 ? bid - tc : -1; e0 = *S(0, k); e1 = *S(0, k + 1);
      } else if (piece == 2) {    // bottom halo row TH <- the tile below's top row
        d0 = S(TH, k); d1 = S(TH, k + 1);
        nb = ty < tr - 1 ? bid + tc : -1; e0 = *S(TH - 1, k); e1 = *S(TH - 1, k + 1);
      } else if (piece < 5) {     // left halo columns -2, -1 <- the left tile's right two columns
        d0 = k < TH ? S(k, piece - 5) : nullptr; d1 = k + 1 < TH ? S(k + 1, piece - 5) : nullptr;
        nb = tx > 0 ? bid - 1 : -1; e0 = *S(k < TH ? k : 0, 0); e1 = *S(k + 1 < TH ? k + 1 : 0, 0);
      } else {                    // right halo column TWv <- the right tile's left column
        d0 = k < TH ? S(k, TWv) : nullptr; d1 = k + 1 < TH ? S(k + 1, TWv) : nullptr;
        nb = tx < tc - 1 ? bid + 1 : -1; e0 = *S(k < TH ? k : 0, TWv - 1); e1 = *S(k + 1 < TH ? k + 1 : 0, TWv - 1);
      }
      if (nb >= 0) {
        const u32x4r_t v = ld_line16(hbn + (size_t)nb * RT_HALO, (unsigned)p * 16u);
        e0 = __longlong_as_double((long long)(((unsigned long long)v.y << 32) | v.x));
        e1 = line16_f64(v);
      }
      if (d0) *d0 = e0;
      if (d1) *d1 = e1;
    };

    if (bid != 0) {
      // ---- an ordinary tile: border, border signal, the neighbours' borders; the release is polled at the top of the next iteration
      for (int p = tid; p < kPairs; p += RT_THREADS) store_border(p);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      stamp(it, kStampIt, 4);                                    // borders have reached memory
      if (tid == 0) st_line16_u64(rs->hflag, (unsigned)bid * 64u, gen, 0u, 0ull);
      if (want_borders) {
        if (tid < 64) {
          const int ok = neighbours_arrived();
          if (lane == 0) { if (!ok) st_agent(&rs->error, 1); s_flag[0] = ok; }
        }
        __syncthreads();
        const int okn = s_flag[0];
        __syncthreads();
        if (!okn) { gave_up = true; break; }
        for (int p = tid; p < kPairs; p += RT_THREADS) fetch(p);
        lds_barrier();       // (the halo ring is complete)
        pre_reads();
      }
    } else {
      // ---- workgroup 0 is the barrier's MASTER, and a tile like any other -- among the last to arrive as often as any other, so nothing of
      // its own may stand between its arrival and its first look at the arrival lines.  Its waves split the work (no workgroup barrier
      // until the release is out):
      //   waves 0-3 POLL: 64 arrival lines each, lane = tile, three 16-byte pieces per line; a wave whose share is complete leaves its
      //     partial sums and the generation in LDS; wave 0 collects the four, books the iteration and releases everybody.  These waves
      //     have no store in flight: memory operations of a wave return in order, and polls issued behind the border stores came back
      //     after 1.4 us instead of 0.8 (profiles/r04_C4/resident_timeline_2048_master_waves.txt);
      //   waves 4-7 WORK: the tile's border stores, the border signal (the last of the four whose stores are acknowledged), the wait for
      //     the tile's own neighbours and the fetch of their borders -- finished long before the release is.
      // (Single-wave code is latency-bound -- 8 cycles an instruction: everything wave 0 does is the critical path of 255 waiting
      // workgroups.)  Round-4 history of this block: DESIGN.md 4.1b.
      constexpr int kPollWaves = RT_WAVES / 2, kWorkThreads = RT_THREADS - 64 * kPollWaves;
      static_assert(64 * kPollWaves >= CVH_RESIDENT_MAX_TILES, "the master's polling waves watch 64 arrival lines each");
      int ok_w = 1;                  // (wave-uniform) this wave's errand went well
      if (wave >= kPollWaves) {
        for (int p = tid - 64 * kPollWaves; p < kPairs; p += kWorkThreads) store_border(p);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0 && __hip_atomic_fetch_add(&s_flag[9], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + 1 == (RT_WAVES - kPollWaves) * (int)gen) {
          if (a.dbg_times && it == kStampIt) a.dbg_times[(size_t)bid * 12 + 4] = __builtin_amdgcn_s_memrealtime();
          st_line16_u64(rs->hflag, (unsigned)bid * 64u, gen, 0u, 0ull);
        }
        if (want_borders) {
          ok_w = neighbours_arrived();
          if (ok_w) for (int p = tid - 64 * kPollWaves; p < kPairs; p += kWorkThreads) fetch(p);
        }
        if (lane == 0 && !ok_w) st_agent(&rs->error, 1);
      } else {
        const int b = wave * 64 + lane;
        const bool have = b < ntiles;
        bool done = false;
        u32x4r_t fa = {0u, 0u, 0u, 0u}, fb = {0u, 0u, 0u, 0u}, fc = {0u, 0u, 0u, 0u};
        u32x4r_t fd = {0u, 0u, 0u, 0u}, fe = {0u, 0u, 0u, 0u};          // three channels: sum I_1 H', sum I_2 H'
        // (one poll in flight: two in flight, half a round trip apart, sample a line twice as often and are SLOWER -- 2048^2 14.60 -> 15.04 us,
        // 1024^2 7.89 -> 8.19: reads of a line that is being written get in the way of the write)
        int rounds = 0;
        bool ok = !have;             // (per lane, sticky: a line that has arrived is not read again -- the last rounds poll the stragglers only)
        for (int round = 0; round < a.res_poll_cap; ++round) {
          if (!ok) {
            fa = ld_line16(rs->flag, (unsigned)b * 16u);
            fb = ld_line16(rs->flag, (CVH_RESIDENT_MAX_TILES + (unsigned)b) * 16u);
            fc = ld_line16(rs->flag, (2u * CVH_RESIDENT_MAX_TILES + (unsigned)b) * 16u);
            if (C == 3) {
              fd = ld_line16(rs->flag, (3u * CVH_RESIDENT_MAX_TILES + (unsigned)b) * 16u);
              fe = ld_line16(rs->flag_c3, (unsigned)b * 16u);
            }
          }
          ok = !have || (tagged(fa) && tagged(fb) && tagged(fc) && (C == 1 || (tagged(fd) && tagged(fe))));
          rounds = round + 1;
          if (__builtin_amdgcn_ballot_w64(!ok) == 0ull) { done = true; break; }
          if ((round & 15) == 15 && ld_agent((const unsigned *)&rs->error) != 0u) break;
          __builtin_amdgcn_s_sleep(kMasterSleep);
        }
        if (a.dbg_times && it == kStampIt && lane == 0) {   // diagnostic: when this wave's share was complete, after how many rounds
          a.dbg_times[(size_t)CVH_RESIDENT_MAX_TILES * 12 + wave] = __builtin_amdgcn_s_memrealtime();
          a.dbg_times[(size_t)CVH_RESIDENT_MAX_TILES * 12 + 8 + wave] = (unsigned long long)rounds;
        }
        if (done) {
          const double ws = wave_sum(have ? line16_f64(fa) : 0.0);                       // fixed order: lane = tile
          const long long r0s = row16_sum_i64(have ? line16_i64(fb) : 0ll), r1s = row16_sum_i64(have ? line16_i64(fc) : 0ll);
          const long long w0 = (read_lane_i64(r0s, 0) + read_lane_i64(r0s, 16)) + (read_lane_i64(r0s, 32) + read_lane_i64(r0s, 48));
          const long long w1 = (read_lane_i64(r1s, 0) + read_lane_i64(r1s, 16)) + (read_lane_i64(r1s, 32) + read_lane_i64(r1s, 48));
          long long w2 = 0, w3 = 0;
          if (C == 3) {
            const long long r2s = row16_sum_i64(have ? line16_i64(fd) : 0ll), r3s = row16_sum_i64(have ? line16_i64(fe) : 0ll);
            w2 = (read_lane_i64(r2s, 0) + read_lane_i64(r2s, 16)) + (read_lane_i64(r2s, 32) + read_lane_i64(r2s, 48));
            w3 = (read_lane_i64(r3s, 0) + read_lane_i64(r3s, 16)) + (read_lane_i64(r3s, 32) + read_lane_i64(r3s, 48));
          }
          if (lane == 0) {
            sred[RT_WAVES * NP + wave * NP] = ws;
            reinterpret_cast<long long *>(sred)[RT_WAVES * NP + wave * NP + 1] = w0;
            reinterpret_cast<long long *>(sred)[RT_WAVES * NP + wave * NP + 2] = w1;
            if (C == 3) {
              reinterpret_cast<long long *>(sred)[RT_WAVES * NP + wave * NP + 3] = w2;
              reinterpret_cast<long long *>(sred)[RT_WAVES * NP + wave * NP + 4] = w3;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __hip_atomic_store(&s_mflag[wave], (int)gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        } else { ok_w = 0; if (lane == 0) st_agent(&rs->error, 1); }
        if (wave == 0 && done) {
          bool all = false;
          for (int round = 0; round < a.res_poll_cap; ++round) {
            const int f = lane < kPollWaves ? __hip_atomic_load(&s_mflag[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : (int)gen;
            if (__builtin_amdgcn_ballot_w64(f != (int)gen) == 0ull) { all = true; break; }
            if ((round & 63) == 63 && ld_agent((const unsigned *)&rs->error) != 0u) break;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          if (all) {
            if (a.dbg_times && it == kStampIt && tid == 0) a.dbg_times[5] = __builtin_amdgcn_s_memrealtime();   // master: everybody has arrived
            // iteration `it` is complete everywhere: norm (fixed order), stop rule (src/main.cpp:993-1000), region means of u(it + 1) from
            // the integer totals
            const double *vred = sred + RT_WAVES * NP;               // (plain LDS reads: the acquire fence above orders them)
            const long long *vredq = reinterpret_cast<const long long *>(sred + RT_WAVES * NP);
            double s4 = vred[0];
            long long q0 = vredq[1], q1 = vredq[2];
            long long qk[C] = {};                                    // three channels: the totals of sum I_1 H', sum I_2 H' in qk[1], qk[2]
#pragma unroll
            for (int ch = 1; ch < C; ++ch) qk[ch] = vredq[2 + ch];
#pragma unroll
            for (int wv = 1; wv < kPollWaves; ++wv) {                // fixed order
              s4 += vred[wv * NP]; q0 += vredq[wv * NP + 1]; q1 += vredq[wv * NP + 2];
#pragma unroll
              for (int ch = 1; ch < C; ++ch) qk[ch] += vredq[wv * NP + 2 + ch];
            }
            const double nrm = sqrt(s4);
            const int stop_now = nrm <= a.stop_cond;          // :1000, after the update
            // chain_means' formula (chain_device.h) on the totals
            // (a NaN norm: u(it + 1) holds a NaN and its means are NaN, as in finalize(), csv_device.h -- through sum H, the divisor of every mean)
            const double sh_fin = __builtin_fma((double)q0, a.chain_inv[0], 0.5 * a.npix);
            const double sh = nrm != nrm ? nrm : sh_fin;
            const double sih = __builtin_fma((double)q1, a.chain_inv[1], 0.5 * a.sum_img[0]);
            // (both quotients through one division sequence in lanes 0 / 1 was tried: norm + means 0.28 -> 0.50 us -- the two sequences overlap as they are)
            const double n1 = sih / sh, n2 = (a.sum_img[0] - sih) / (a.npix - sh);
            double nk1[C] = {}, nk2[C] = {};                          // three channels: the means of channels 1, 2
#pragma unroll
            for (int ch = 1; ch < C; ++ch) {
              const double sihk = __builtin_fma((double)qk[ch], a.chain_inv[1 + ch], 0.5 * a.sum_img[ch]);
              nk1[ch] = sihk / sh; nk2[ch] = (a.sum_img[ch] - sihk) / (a.npix - sh);
            }
            const unsigned leave = (stop_now || it + 1 >= nit) ? 1u : 0u;
            stamp(it, kStampIt, 6);                                  // master: norm and means known
            if (C == 1) {
              for (int i = lane, nl = go_lines(ntiles, a.res_go_shift); i < nl; i += 64) {
                st_line16(rs->go, (unsigned)i * 64u, gen, leave, n1);
                st_line16(rs->go, (unsigned)i * 64u + 16u, gen, leave, n2);
              }
            } else {                                                 // six pieces on a 128-byte line, every piece with its generation
              for (int i = lane, nl = go_lines(ntiles, a.res_go_shift); i < nl; i += 64) {
                st_line16(rs->go_c3, (unsigned)i * 128u, gen, leave, n1);
                st_line16(rs->go_c3, (unsigned)i * 128u + 48u, gen, leave, n2);
#pragma unroll
                for (int ch = 1; ch < C; ++ch) {
                  st_line16(rs->go_c3, (unsigned)i * 128u + 16u * (unsigned)ch, gen, leave, nk1[ch]);
                  st_line16(rs->go_c3, (unsigned)i * 128u + 48u + 16u * (unsigned)ch, gen, leave, nk2[ch]);
                }
              }
            }
            stamp(it, kStampIt, 7);                                  // master: release issued
            own.gen = (int)gen; own.leave = (int)leave; own.c1[0] = n1; own.c2[0] = n2;
#pragma unroll
            for (int ch = 1; ch < C; ++ch) { own.c1[ch] = nk1[ch]; own.c2[ch] = nk2[ch]; }
            // everything else the master books comes AFTER the release (off the critical path of the other workgroups).
            // The last iteration of the launch leaves the sums where the per-launch path expects them: set p0 + executed filled (one
            // shard per sum), the set behind it clear
            if (leave) {
              // (a set is (1 + C) sums x 64 / (1 + C) shards, chain_device.h: one channel's sums sit at lanes 0 / 32, three channels' at 0 / 16 / 32 / 48)
              if (C == 1)
                __hip_atomic_store(&a.chain->v[(phase + 1) & 3][lane], lane == 0 ? q0 : lane == 32 ? q1 : 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              else
                __hip_atomic_store(&a.chain->v[(phase + 1) & 3][lane], lane == 0 ? q0 : lane == 16 ? q1 : lane == 32 ? qk[C > 1 ? 1 : 0] : lane == 48 ? qk[C > 2 ? 2 : 0] : 0ll,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_store(&a.chain->v[(phase + 2) & 3][lane], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // (inside a launch the books are written behind the workgroup's meeting below: on gfx9 a wave's stores count in vmcnt like its
            // loads, and every conservative `s_waitcnt vmcnt(0)` on wave 0's way into the next iteration would wait for them)
            if (leave) book(cm1, cm2, nrm, stop_now, true);
            else { book_pending = true; book_nrm = nrm; }
          } else if (lane == 0) st_agent(&rs->error, 1);
        }
        // (a master that gave up has raised the error word and released nobody: every wait below and in the other workgroups sees the
        // word and leaves)
      }
      // the eight waves meet ONCE, behind the release, and thread 0 hands over what it wrote: the master tile polls no release line and
      // has no round trip left on its way into the next iteration (it used to be the LAST tile into every iteration, 1.3 us behind the median)
      if (lane == 0) s_flag[wave] = ok_w;
      if (tid == 0) {
        s_bc[0] = (double)(own.gen == (int)gen ? own.leave : -1); s_bc[1] = own.c1[0]; s_bc[2] = own.c2[0];
#pragma unroll
        for (int ch = 1; ch < C; ++ch) { s_bc[1 + 2 * ch] = own.c1[ch]; s_bc[2 + 2 * ch] = own.c2[ch]; }
      }
      lds_barrier();
      int okn = 1;
#pragma unroll
      for (int wv = 0; wv < RT_WAVES; ++wv) okn &= s_flag[wv];
      go_known = (int)s_bc[0];
      const double k1 = s_bc[1], k2 = s_bc[2];
      double kk1[C] = {}, kk2[C] = {};
#pragma unroll
      for (int ch = 1; ch < C; ++ch) { kk1[ch] = s_bc[1 + 2 * ch]; kk2[ch] = s_bc[2 + 2 * ch]; }
      lds_barrier();
      if (!okn || go_known < 0) { gave_up = true; break; }   // (a neighbour or the master's own collection gave up: the error word is up)
      if (book_pending) { book(cm1, cm2, book_nrm, 0, false); book_pending = false; }   // (c1 / c2: still the means this iteration ran with)
      if (want_borders) {                                      // (the workers' fetch lies in front of the meeting's first barrier)
        c1 = k1; c2 = k2;
#pragma unroll
        for (int ch = 1; ch < C; ++ch) { cm1[ch] = kk1[ch]; cm2[ch] = kk2[ch]; }
        pre_reads();
      }
      have_go = true;
    }
  }
  if (gave_up) return;
  // ---- leave: every workgroup waits for the release behind the last iteration it computed (the whole grid has then finished it),
  // then writes its tile back into the ping-pong buffer the per-launch path would hold the result in
  if (executed > 0) {
    double d1[C], d2[C];
    if (wg_wait_go<C>(rs, bid, executed, a, s_bc, d1, d2, own) < 0) return;
  }
  // (an even count lands in the buffer the launch read from: every workgroup has long finished reading it -- the first grid
  // barrier lies behind all the tile loads)
  double *const dst = (executed & 1) ? a.u_out : const_cast<double *>(a.u_in);
  if (executed > 0) {
    for (int q = tid; q < TH * (RT_W / 2); q += RT_THREADS) {
      const int r = q / (RT_W / 2), c = 2 * (q % (RT_W / 2));
      if (c < TWv) *reinterpret_cast<double2_t *>(dst + (size_t)(r0 + r) * w + c0 + c) = *reinterpret_cast<const double2_t *>(S(r, c));
    }
  }
