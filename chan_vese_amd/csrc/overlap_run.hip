// overlap_run.hip — host side of cvh_overlaps* (include/chanvese_hip.h, "Component overlaps"): the contingency table of the components of
// the masks of n contexts, raw or cleaned, against a second label plane each -- ONE MemberCall (cvh_host.h, io_run.hip) with two member
// tables, as measure_run.hip: the mask source's (MaskSource, components_run.hip) for the cleaning and numbering launches, and a second one
// for overlap_kernels.hip.  The single-context forms are batches of one; the host form stages its plane on the context's stream and is
// then the device form on that stream.  The pair table of a member lives in the context (overlap) and keeps the size it has grown to:
// a launch whose table overflows is run again, for the members concerned, on a table four times as large.  The rows come down in slot
// order and are SORTED HERE, behind the wait for them.  The calls only read: nothing of a member's level set, run state, sums, options
// or planes is assigned here.  cvh_match_overlaps, the host arithmetic on a table, lives here too.
#include "cvh_host.h"

namespace {

constexpr size_t kFirstSlots = 4096;   // 96 KiB with the rows: 2048 pairs before the first growth
constexpr size_t kSlotBytes = sizeof(CvhOverlapSlot), kRowBytes = sizeof(cvh_overlap);

// the table no plane of n pixels overflows: more than twice the n pairs it can have
size_t max_slots(size_t n)
{
  size_t s = kFirstSlots;
  while (s / 2 <= n) s *= 2;
  return s;
}

// c's table has `slots` slots, and half as many rows behind them, afterwards
int set_slots(cvh_context *lead, cvh_context *c, size_t slots)
{
  return grow_table_to(lead, &c->overlap, slots, slots, slots * kSlotBytes + slots / 2 * kRowBytes);
}

bool row_less(const cvh_overlap &x, const cvh_overlap &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; }

int overlaps(cvh_context *const *ctxs, int n, const MaskSource &src, const int32_t *const *d_others, cvh_overlap *const *tables, const long *caps,
             long *pairs, int *counts, void *stream, const char *what)
{
  int rc = src.check(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (!d_others) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of device pointers is NULL", what);
  rc = members_caps_fit(ctxs, n, what, (const void *const *)tables, caps, "cap", "tables without caps");
  if (rc == CVH_OK) rc = members_below(ctxs, n, what, 31);   // (a count fits 32 bits)
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) {
    rc = element_pointer_check(ctxs, n, i, d_others[i], sizeof(int32_t), what);
    if (rc != CVH_OK) return rc;
  }
  rc = src.ready(ctxs, n, what, true);
  if (rc != CVH_OK) return rc;
  const bool cleaned = src.cleaned();
  std::vector<void *> masks((size_t)n, nullptr);
  std::vector<size_t> want_rows((size_t)n, 0);   // rows the caller has room for
  bool any_rows = false;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    if (cleaned) {   // the cleaned mask goes to the context's own mask buffer (cvh_get_mask's) and is labelled there
      if (!c->d_mask) HIPCHK(lead, hipMalloc((void **)&c->d_mask, c->n));
      masks[(size_t)i] = c->d_mask;
    }
    rc = set_slots(lead, c, kFirstSlots);   // (the first call's: a table that exists has at least as many)
    if (rc != CVH_OK) return rc;
    if (tables && tables[i] && caps[i] > 0) { want_rows[(size_t)i] = (size_t)caps[i]; any_rows = true; }
  }
  // staging: [the mask launches' table][the pair launches' table][one word per member][CVH_OVERLAP_CTL control words per member], zero
  const size_t word_bytes = (size_t)n * sizeof(unsigned long long), ctl_bytes = (size_t)n * CVH_OVERLAP_CTL * sizeof(unsigned);
  MemberCall call;
  rc = call.begin(ctxs, n, what, word_bytes + ctl_bytes, 0, true);
  if (rc != CVH_OK) return rc;
  unsigned char *const d_ctl = call.db + call.extra_off + word_bytes;
  const unsigned long long *words = (const unsigned long long *)(call.hb + call.extra_off);
  const unsigned *ctl = (const unsigned *)(call.hb + call.extra_off + word_bytes);
  auto point_at_table = [&](int i) {
    const cvh_context *c = ctxs[i];
    CvhIoMember &m = call.tab2[i];
    m.dst = c->overlap.d;
    m.plane[0] = (uint8_t *)c->overlap.d + c->overlap.count * kSlotBytes;
    m.src_stride = c->overlap.count;
  };
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    src.fill(&call, i, masks[(size_t)i], (unsigned long long *)(call.db + call.extra_off) + i, true);
    CvhIoMember &m = call.tab2[i];
    m.src = c->d_cc;
    m.src2 = d_others[i];
    m.sums = (unsigned long long *)(d_ctl + (size_t)i * CVH_OVERLAP_CTL * sizeof(unsigned));
    m.w2 = want_rows[(size_t)i] ? 1 : 0;
    m.nblk = cvh_measure_blocks(c->n);
    point_at_table(i);
  }
  // the pair launch for the members that do not sit out, and what it leaves: K, and per member {P, overflow, rows written}
  auto pair_launch = [&]() -> int {
    for (int i = 0; i < n; ++i)
      if (!call.tab2[i].h2) HIPCHK(lead, hipMemsetAsync(ctxs[i]->overlap.d, 0, ctxs[i]->overlap.count * kSlotBytes, lead->stream));
    HIPCHK(lead, cvh_launch_overlap(call.dtab2(), n, call.grid2, any_rows, lead->stream));
    ++g_launches[kOverlapLaunchSets];
    HIPCHK(lead, hipMemcpyAsync((void *)words, call.db + call.extra_off, word_bytes + ctl_bytes, hipMemcpyDeviceToHost, lead->stream));
    return CVH_OK;
  };
  rc = call.run(stream, false, true, [&]() -> int {   // the first host wait of the call: K and P
    const int rc_mask = src.launch(call, false);
    if (rc_mask != CVH_OK) return rc_mask;
    HIPCHK(lead, cvh_launch_cc_number(call.dtab(), n, call.grid, cleaned ? 1 : 0, src.conn, src.invert, lead->stream));
    return pair_launch();
  });
  if (rc != CVH_OK) return rc;
  // a member whose table overflowed takes one four times as large (never beyond what no plane of its size overflows) and the pair
  // launch runs again for those members alone: one more host wait per round
  for (;;) {
    bool again = false;
    for (int i = 0; i < n; ++i) {
      cvh_context *c = ctxs[i];
      const bool over = !call.tab2[i].h2 && ctl[(size_t)i * CVH_OVERLAP_CTL + 1] != 0;
      call.tab2[i].h2 = over ? 0 : 1;
      if (!over) continue;
      if (c->overlap.count >= max_slots(c->n))
        return batch_fail(ctxs, n, CVH_ERR_HIP, "%s: member %d: the pair table of %zu slots overflowed", what, i, c->overlap.count);
      rc = set_slots(lead, c, std::min(c->overlap.count * 4, max_slots(c->n)));
      if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, std::string(lead->err).c_str());
      point_at_table(i);
      HIPCHK(lead, hipMemsetAsync((void *)call.tab2[i].sums, 0, CVH_OVERLAP_CTL * sizeof(unsigned), lead->stream));
      again = true;
    }
    if (!again) break;
    rc = call.upload_again(call.tab2);
    if (rc == CVH_OK) rc = pair_launch();
    if (rc == CVH_OK) rc = call.wait_again(stream, false);
    if (rc != CVH_OK) return rc;
  }
  // the rows: P is known now; they come down unsorted (the SECOND wait, only where rows are asked for) and are sorted here
  std::vector<std::vector<cvh_overlap>> rows((size_t)n);
  bool fetch = false;
  for (int i = 0; i < n; ++i) {
    const size_t P = ctl[(size_t)i * CVH_OVERLAP_CTL];
    if (!want_rows[(size_t)i] || !P) continue;
    if (ctl[(size_t)i * CVH_OVERLAP_CTL + 2] != P)
      return batch_fail(ctxs, n, CVH_ERR_HIP, "%s: member %d: %u rows written for %zu pairs", what, i, ctl[(size_t)i * CVH_OVERLAP_CTL + 2], P);
    rows[(size_t)i].resize(P);
    HIPCHK(lead, hipMemcpyAsync(rows[(size_t)i].data(), (const uint8_t *)ctxs[i]->overlap.d + ctxs[i]->overlap.count * kSlotBytes, P * kRowBytes,
                                hipMemcpyDeviceToHost, lead->stream));
    fetch = true;
  }
  if (fetch) {
    rc = call.wait_again(stream, false);
    if (rc != CVH_OK) return rc;
  }
  for (int i = 0; i < n; ++i) {
    std::vector<cvh_overlap> &r = rows[(size_t)i];
    if (r.empty()) continue;
    std::sort(r.begin(), r.end(), row_less);
    memcpy(tables[i], r.data(), std::min(r.size(), want_rows[(size_t)i]) * kRowBytes);
  }
  for (int i = 0; i < n; ++i) {
    if (pairs) pairs[i] = (long)ctl[(size_t)i * CVH_OVERLAP_CTL];
    if (counts) counts[i] = (int)words[i];
  }
  return CVH_OK;
}

}  // namespace

extern "C" int cvh_overlaps_device_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                         const int32_t *const *d_others, cvh_overlap *const *tables, const long *caps, long *pairs,
                                         int *counts, void *stream)
{
  static const char what[] = "cvh_overlaps_device_batch";
  return guarded(ctxs, n, what, [&]() {
    return overlaps(ctxs, n, {conn, invert, min_area, fill_holes, keep_largest}, d_others, tables, caps, pairs, counts, stream, what);
  });
}

extern "C" int cvh_overlaps_device(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                   const int32_t *d_other, cvh_overlap *table, long cap, long *pairs, int *count, void *stream)
{
  return guarded_one(c, "cvh_overlaps_device", [&](const char *what) {
    return overlaps(&c, 1, {conn, invert, min_area, fill_holes, keep_largest}, &d_other, &table, &cap, pairs, count, stream, what);
  });
}

extern "C" int cvh_overlaps(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, const int32_t *other,
                            cvh_overlap *table, long cap, long *pairs, int *count)
{
  return guarded_one(c, "cvh_overlaps", [&](const char *what) {
    const MaskSource src = {conn, invert, min_area, fill_holes, keep_largest};
    int rc = src.check(&c, 1, what);
    if (rc != CVH_OK) return rc;
    if (!other) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: other is NULL", what);
    if (table && cap < 0) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: member 0: cap must not be negative, got %ld", what, cap);
    if (c->n >= ((size_t)1 << 31)) return members_below(&c, 1, what, 31);
    if (!c->have_u) return members_have_levelsets(&c, 1, what);   // before the plane is allocated
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_workspace(c, &c->d_overlap_plane, c->n * sizeof(int32_t), "overlap plane", false);
    if (rc != CVH_OK) return batch_fail(&c, 1, rc, "%s: %s", what, std::string(c->err).c_str());
    // the plane rides the context's stream (as cvh_score_mask's bytes: read by this call's launches alone, which the same stream orders
    // behind the copy and, by the call's host wait, in front of the next call's copy)
    HIPCHK(c, hipMemcpyAsync(c->d_overlap_plane, other, c->n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const int32_t *d_other = (const int32_t *)c->d_overlap_plane;
    return overlaps(&c, 1, src, &d_other, &table, &cap, pairs, count, c->stream, what);
  });
}

extern "C" int cvh_match_overlaps(const cvh_overlap *table, long pairs, uint32_t num, uint32_t den, int32_t *match_of_a, int k, cvh_match *out)
{
  if (!out || pairs < 0 || (pairs > 0 && !table) || k < 0) return CVH_ERR_ARG;
  if (den == 0 || den > 65535 || num > den || 2ull * num < den) return CVH_ERR_ARG;
  try {
    int32_t max_a = 0;
    std::vector<std::pair<int32_t, uint64_t>> by_b;   // (b, count) of every row, then (b, area_b) of every distinct b, ascending
    by_b.reserve((size_t)pairs);
    for (long i = 0; i < pairs; ++i) {
      const cvh_overlap &r = table[i];
      if (r.count == 0 || r.a < 0) return CVH_ERR_ARG;
      if (i > 0 && !row_less(table[i - 1], r)) return CVH_ERR_ARG;   // not in the defined order, or a pair twice
      max_a = std::max(max_a, r.a);
      by_b.emplace_back(r.b, r.count);
    }
    if (match_of_a && k < max_a) return CVH_ERR_ARG;
    std::sort(by_b.begin(), by_b.end());
    size_t nb = 0;
    for (size_t i = 0; i < by_b.size(); ++i) {
      if (nb && by_b[nb - 1].first == by_b[i].first) by_b[nb - 1].second += by_b[i].second;
      else by_b[nb++] = by_b[i];
    }
    by_b.resize(nb);
    cvh_match m;
    memset(&m, 0, sizeof(m));
    for (const auto &e : by_b) m.objects_b += e.first != 0;
    for (int i = 0; match_of_a && i < k; ++i) match_of_a[i] = 0;
    for (long i = 0; i < pairs;) {
      long j = i;
      uint64_t area_a = 0;
      for (; j < pairs && table[j].a == table[i].a; ++j) area_a += table[j].count;
      if (table[i].a != 0) {
        ++m.objects_a;
        for (long q = i; q < j; ++q) {
          const cvh_overlap &r = table[q];
          if (r.b == 0) continue;
          const uint64_t area_b = std::lower_bound(by_b.begin(), by_b.end(), std::make_pair(r.b, (uint64_t)0))->second;
          if ((uint64_t)r.count * den > (uint64_t)num * (area_a + area_b - r.count)) {   // IoU > num / den: at most one b per a, and the reverse
            ++m.tp;
            if (match_of_a) match_of_a[r.a - 1] = r.b;
          }
        }
      }
      i = j;
    }
    m.fp = m.objects_a - m.tp;
    m.fn = m.objects_b - m.tp;
    *out = m;
    return CVH_OK;
  } catch (...) { return CVH_ERR_NOMEM; }
}
