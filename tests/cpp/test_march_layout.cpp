// test_march_layout.cpp — the device-free part of the marching-wave call sequence (chan_vese_amd/csrc/march_flow.h) over synthetic
// records: class sorting, the lay-out of one and of two launch grids, and the loop over the classes present.  Classes of 0, 1 and 3
// records; every `first` is the sum of the grids in front of it in its class, every class's grid the sum over the class.
// chan_vese_amd/host/Makefile builds it into bin/ (tests/test_march_layout.py runs it); under the host sanitizers:
//   make -C chan_vese_amd/host SANITIZE=-fsanitize=address,undefined ../../bin/test_march_layout && bin/test_march_layout
#include "march_flow.h"

namespace {

struct Rec { int member; unsigned grid, grid2, first, first2; };

int failures = 0;
#define EXPECT(cond)                                                           \
  do {                                                                         \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// members 0 .. n-1 of classes class_of[i], member i with grids 10 + i and 100 + 7 i; two: both grids are laid out
void check(const std::vector<int> &class_of, bool two)
{
  const int n = (int)class_of.size();
  std::vector<int> order;
  MarchClass cls[kMarchClasses];
  march_classes(n, [&](int i) { return class_of[i]; }, &order, cls);
  EXPECT((int)order.size() == n);
  std::vector<Rec> recs((size_t)n);
  for (int r = 0; r < n; ++r) recs[r] = Rec{order[r], 10u + order[r], 100u + 7u * order[r], 9999u, 9999u};
  march_lay_out(recs.data(), cls, [&](Rec &r) { return MarchSections{{&r.first, two ? &r.first2 : nullptr}, {r.grid, r.grid2}}; });
  int at = 0, visited = 0;
  for (int k = 0; k < kMarchClasses; ++k) {
    const int want_n = (int)std::count(class_of.begin(), class_of.end(), k);
    EXPECT(cls[k].first == at && cls[k].n == want_n && cls[k].C == (k < 2 ? 1 : 3) && cls[k].fast == (k & 1));
    unsigned sum = 0, sum2 = 0;
    for (int r = at; r < at + want_n; ++r) {
      EXPECT(class_of[recs[r].member] == k);
      EXPECT(r == at || recs[r - 1].member < recs[r].member);   // member order inside a class
      EXPECT(recs[r].first == sum && recs[r].first2 == (two ? sum2 : 9999u));
      sum += recs[r].grid; sum2 += recs[r].grid2;
    }
    EXPECT(cls[k].grid == sum && cls[k].grid2 == (two ? sum2 : 0u));
    at += want_n;
  }
  EXPECT(at == n);
  const int rc = march_each_class((const Rec *)recs.data(), cls, [&](const Rec *tab, const MarchClass &q) {
    EXPECT(q.n > 0 && tab == recs.data() + q.first && class_of[tab[0].member] == (int)(&q - cls));
    visited += q.n;
    return CVH_OK;
  });
  EXPECT(rc == CVH_OK && visited == n);
  EXPECT(march_each_class((const Rec *)recs.data(), cls, [&](const Rec *, const MarchClass &) { return CVH_ERR_ARG; }) == CVH_ERR_ARG);
}

}  // namespace

int main()
{
  for (const bool two : {false, true}) {
    check({2, 0, 2, 2}, two);      // classes of 1, 0, 3, 0 records
    check({3, 3, 1, 3, 0}, two);   // 1, 1, 0, 3
    check({1}, two);               // the one member of a single call: first = 0
  }
  if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
  printf("march lay-out ok\n");
  return 0;
}
