// components_kernels.hip — connected components of the mask (cvh_components*, cvh_get_mask_clean*; gfx950).  Everything is integers; the
// launches are ordered by their kernel boundaries alone -- no workgroup waits for or polls another -- and each is ONE grid over N members
// of mixed shapes (CvhIoMember; a member's section is ceil(h w / 256) workgroups, a lane per pixel in flat raster order, so a wave holds
// 64 consecutive flat indices).
// UNION-FIND with the minimum flat index as root: parent[p] <= p always, a root has parent[p] == p, a pixel outside the class kNone.
//   cc_init_kernel     classifies (the level set by cvh_get_mask's rule, or the bytes of a mask, or their complement) and links every
//                      pixel to the start of its horizontal run inside its wave (ballot + clz: no memory traffic); clears the statistics.
//   cc_merge_kernel    unites a pixel with its left neighbour where the run was cut by a wave boundary, with the pixel above, and for
//                      8-connectivity with the two diagonal pixels above -- only the pairs that are not already implied by other pairs.
//   cc_flatten_*       parent[p] = root(p).  The roots are the components' smallest flat indices WHATEVER the timing was: a link only
//                      ever goes to a smaller index of the same component, so the smallest index of a component never gets a parent and
//                      every other member of the finished tree does.  Labels, table and clean mask are functions of the roots alone.
// Numbering (cvh_components): roots counted per workgroup, one workgroup per member scans the counts, the roots take their numbers in
// raster order (root p then holds kNumbered | k), the labels follow.  The table (after the host knows K) is filled per horizontal run.
// Cleaning (cvh_get_mask_clean*): area (and "touches the border") per root in stat[root], a 64-bit atomic max finds the largest component.
#include "cc_device.h"

namespace {

#define CVH_GLOBAL __attribute__((address_space(1)))
typedef CVH_GLOBAL unsigned *gwords;

static_assert(CVH_BLOCK == 256, "the per-wave counts below are summed as four waves");
constexpr unsigned kNone = kCcNone, kNumbered = kCcNumbered;   // (cc_device.h)
constexpr unsigned kBorder = 0x80000000u;     // stat[root]: the component has a pixel in the first / last row / column (areas are < 2^31)

// the member whose section holds this workgroup (reinit_kernels.hip's reinit_member)
__device__ __forceinline__ int cc_member(const CvhIoMember *tab, int nmem)
{
  int lo = 0, hi = nmem - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct Pixel { const CvhIoMember *m; unsigned p, n; bool live; };
__device__ __forceinline__ Pixel cc_pixel(const CvhIoMember *tab, int nmem)
{
  Pixel x;
  x.m = tab + cc_member(tab, nmem);
  x.n = (unsigned)x.m->n;   // (h w < 2^31)
  x.p = (blockIdx.x - x.m->first) * CVH_BLOCK + threadIdx.x;
  x.live = x.p < x.n;
  return x;
}

__device__ __forceinline__ unsigned ld(gwords a, unsigned i) { return __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Terminates: every step goes to parent[x] < x (a link only ever goes to a smaller index), so x strictly decreases and is bounded by 0.
// A value read late is an earlier parent of x: still an index of x's component, still < x.
__device__ __forceinline__ unsigned cc_find(gwords parent, unsigned x)
{
  for (;;) {
    const unsigned y = ld(parent, x);
    if (y == x) return x;
    x = y;
  }
}

// Terminates: with a > b, the atomic min either finds a a root (old == a: linked, done) or returns old < a, and the loop goes on with the
// pair (old, b) -- a's earlier parent, which the min may just have replaced by b, still has to meet b.  max(a, b) strictly decreases.
__device__ __forceinline__ void cc_union(gwords parent, unsigned a, unsigned b)
{
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) { const unsigned t = a; a = b; b = t; }
    const unsigned old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ unsigned long long upto(unsigned lane) { return (2ull << lane) - 1ull; }   // bits 0 .. lane (lane 63: all)

// mode 0: the class of the level set, ((float)u > 0) != invert; 1: mask byte set; 2: mask byte clear (the mask is the member's dst)
__global__ void __launch_bounds__(CVH_BLOCK) cc_init_kernel(const CvhIoMember *tab, int nmem, int mode, int invert)
{
  const Pixel x = cc_pixel(tab, nmem);
  bool in = false;
  if (x.live) {
    if (mode == 0) in = (((float)((CVH_GLOBAL const double *)x.m->src)[x.p] > 0.0f) ? 1 : 0) != invert;   // cvh_get_mask's rule
    else in = (((CVH_GLOBAL const uint8_t *)x.m->dst)[x.p] != 0) == (mode == 1);
  }
  const unsigned col = x.live ? x.p % (unsigned)x.m->w : 1u;
  const unsigned long long bits = __ballot(in), row0 = __ballot(x.live && col == 0);
  if (!x.live) return;
  unsigned v = kNone;
  if (in) {
    const unsigned long long starts = bits & (~(bits << 1) | row0);   // lane 0 always starts a run
    const unsigned lane = lane_id(), s = 63u - (unsigned)__builtin_clzll(starts & upto(lane));
    v = x.p - (lane - s);
  }
  ((gwords)x.m->plane[0])[x.p] = v;
  ((gwords)x.m->plane[1])[x.p] = 0;
}

__global__ void __launch_bounds__(CVH_BLOCK) cc_merge_kernel(const CvhIoMember *tab, int nmem, int conn)
{
  const Pixel x = cc_pixel(tab, nmem);
  if (!x.live) return;
  const gwords parent = (gwords)x.m->plane[0];
  if (ld(parent, x.p) == kNone) return;
  const unsigned w = (unsigned)x.m->w, p = x.p, r = p / w, c = p % w;
  // (whether a pixel is of the class never changes: only WHICH index its word holds does)
  const bool left = c > 0 && ld(parent, p - 1) != kNone, up = r > 0 && ld(parent, p - w) != kNone;
  const bool upleft = r > 0 && c > 0 && ld(parent, p - w - 1) != kNone;
  if (left && lane_id() == 0) cc_union(parent, p, p - 1);   // inside a wave cc_init_kernel linked the run
  // left and up-left both set: (left, up-left) is a vertical pair of its own, and the two horizontal pairs close the square
  if (up && !(left && upleft)) cc_union(parent, p, p - w);
  if (conn == 8 && r > 0 && !up) {   // (up set: the pixel above is joined to both diagonal ones horizontally)
    if (upleft && !left) cc_union(parent, p, p - w - 1);   // (left set: up-left is the pixel above it)
    if (c + 1 < w && ld(parent, p - w + 1) != kNone) cc_union(parent, p, p - w + 1);
  }
}

// the root of a pixel of the class, kNone for the others; the pixel's word is flattened to it
__device__ __forceinline__ unsigned cc_flatten(const Pixel &x)
{
  if (!x.live) return kNone;
  const gwords parent = (gwords)x.m->plane[0];
  if (ld(parent, x.p) == kNone) return kNone;
  const unsigned root = cc_find(parent, x.p);
  parent[x.p] = root;   // (a lane that walks through p meanwhile reads the old parent or the root: both lead to the root)
  return root;
}

// cvh_components: flatten, and count the roots of the workgroup
__global__ void __launch_bounds__(CVH_BLOCK) cc_flatten_count_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned cnt[CVH_BLOCK / 64];
  const Pixel x = cc_pixel(tab, nmem);
  const unsigned root = cc_flatten(x);
  const unsigned long long roots = __ballot(root != kNone && root == x.p);
  if (lane_id() == 0) cnt[threadIdx.x >> 6] = (unsigned)__builtin_popcountll(roots);
  __syncthreads();
  if (threadIdx.x == 0) ((gwords)x.m->plane[2])[blockIdx.x - x.m->first] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// one workgroup per member: the counts become the number of roots before the workgroup; K goes to the member's word
__global__ void __launch_bounds__(CVH_BLOCK) cc_scan_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned part[CVH_BLOCK];
  const CvhIoMember *m = tab + blockIdx.x;
  const gwords cnt = (gwords)m->plane[2];
  const unsigned nb = m->nblk, chunk = (nb + CVH_BLOCK - 1) / CVH_BLOCK;
  const unsigned lo = threadIdx.x * chunk < nb ? threadIdx.x * chunk : nb, hi = lo + chunk < nb ? lo + chunk : nb;
  unsigned mine = 0;
  for (unsigned i = lo; i < hi; ++i) mine += cnt[i];
  part[threadIdx.x] = mine;
  __syncthreads();
  unsigned before = 0;
  for (unsigned t = 0; t < threadIdx.x; ++t) before += part[t];
  for (unsigned i = lo; i < hi; ++i) { const unsigned v = cnt[i]; cnt[i] = before; before += v; }
  if (threadIdx.x == CVH_BLOCK - 1) *m->sums = before;
}

// the roots take their numbers, in raster order
__global__ void __launch_bounds__(CVH_BLOCK) cc_number_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned cnt[CVH_BLOCK / 64];
  const Pixel x = cc_pixel(tab, nmem);
  const gwords parent = (gwords)x.m->plane[0];
  const bool root = x.live && parent[x.p] == x.p;
  const unsigned long long roots = __ballot(root);
  const unsigned wave = threadIdx.x >> 6;
  if (lane_id() == 0) cnt[wave] = (unsigned)__builtin_popcountll(roots);
  __syncthreads();
  if (!root) return;
  unsigned k = ((gwords)x.m->plane[2])[blockIdx.x - x.m->first] + 1u + (unsigned)__builtin_popcountll(roots & (upto(lane_id()) >> 1));
  for (unsigned v = 0; v < wave; ++v) k += cnt[v];
  parent[x.p] = kNumbered | k;
}

// the number of a pixel's component after cc_number_kernel, 0 outside the class
__device__ __forceinline__ unsigned cc_number(gwords parent, unsigned p)
{
  const unsigned v = parent[p];
  if (v == kNone) return 0;
  return ((v & kNumbered) ? v : parent[v]) & ~kNumbered;
}

__global__ void __launch_bounds__(CVH_BLOCK) cc_labels_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = cc_pixel(tab, nmem);
  if (!x.live || !x.m->dst) return;   // (a member without a label plane: wave-uniform)
  ((CVH_GLOBAL int *)x.m->dst)[x.p] = (int)cc_number((gwords)x.m->plane[0], x.p);
}

// table rows (the member's dst in these two launches): a root writes `first` and the neutral elements of the sums
__global__ void __launch_bounds__(CVH_BLOCK) cc_table_init_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = cc_pixel(tab, nmem);
  if (!x.live) return;
  const unsigned v = ((gwords)x.m->plane[0])[x.p];
  if (v == kNone || !(v & kNumbered)) return;
  CVH_GLOBAL cvh_component *row = (CVH_GLOBAL cvh_component *)x.m->dst + ((v & ~kNumbered) - 1u);
  cc_row_init(row, x.p);
}

__device__ __forceinline__ unsigned run_length(unsigned key, bool cut) { return cc_run_length(key, cut); }   // (cc_device.h)

// area and box per component: one set of atomics per horizontal run inside a wave; min and max only where they would move the value
__global__ void __launch_bounds__(CVH_BLOCK) cc_table_stats_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = cc_pixel(tab, nmem);
  const unsigned w = (unsigned)x.m->w, k = x.live ? cc_number((gwords)x.m->plane[0], x.p) : 0u;
  const unsigned c = x.live ? x.p % w : 1u;
  const unsigned len = run_length(k ? k : kNone, c == 0);
  if (!len) return;
  CVH_GLOBAL cvh_component *row = (CVH_GLOBAL cvh_component *)x.m->dst + (k - 1u);
  cc_row_add_run(row, len, (int)(x.p / w), (int)c);
}

// cleaning: flatten, and add the areas into stat[root], one add per run of a root inside a wave; border = 1 also marks the roots whose
// component touches the first / last row / column
__global__ void __launch_bounds__(CVH_BLOCK) cc_flatten_area_kernel(const CvhIoMember *tab, int nmem, int border)
{
  const Pixel x = cc_pixel(tab, nmem);
  const unsigned root = cc_flatten(x);
  const unsigned len = run_length(root, false);
  const gwords stat = (gwords)x.m->plane[1];
  if (len) __hip_atomic_fetch_add(stat + root, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (border && root != kNone) {
    const unsigned w = (unsigned)x.m->w, h = (unsigned)x.m->h, r = x.p / w, c = x.p % w;
    if ((r == 0 || r == h - 1 || c == 0 || c == w - 1) && !(ld(stat, root) & kBorder))
      __hip_atomic_fetch_or(stat + root, kBorder, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// keep_largest: the roots bid {area, smaller first wins a tie} for the member's word (zeroed by the host)
__global__ void __launch_bounds__(CVH_BLOCK) cc_largest_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = cc_pixel(tab, nmem);
  if (!x.live || ((gwords)x.m->plane[0])[x.p] != x.p) return;
  const unsigned long long bid = ((unsigned long long)((gwords)x.m->plane[1])[x.p] << 32) | (unsigned long long)(0xffffffffu - x.p);
  CVH_GLOBAL unsigned long long *best = (CVH_GLOBAL unsigned long long *)x.m->sums;
  if (bid > __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_max(best, bid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the bytes of the mask (the member's dst).  step 1: mask = class and area >= a;  2: the pixels of the (complement) class whose component
// does not touch the border and has area <= a are set;  3: the pixels of the class outside the largest component are cleared
__global__ void __launch_bounds__(CVH_BLOCK) cc_write_kernel(const CvhIoMember *tab, int nmem, int step, unsigned a)
{
  const Pixel x = cc_pixel(tab, nmem);
  if (!x.live) return;
  const unsigned root = ((gwords)x.m->plane[0])[x.p];
  CVH_GLOBAL uint8_t *mask = (CVH_GLOBAL uint8_t *)x.m->dst;
  if (step == 1) { mask[x.p] = (root != kNone && ((gwords)x.m->plane[1])[root] >= a) ? 1 : 0; return; }
  if (root == kNone) return;
  if (step == 2) {
    const unsigned s = ((gwords)x.m->plane[1])[root];
    if (!(s & kBorder) && s <= a) mask[x.p] = 1;
  } else {
    const unsigned long long best = *(CVH_GLOBAL const unsigned long long *)x.m->sums;
    if (root != 0xffffffffu - (unsigned)best) mask[x.p] = 0;
  }
}

}  // namespace

unsigned cvh_cc_blocks(size_t n) { return (unsigned)((n + CVH_BLOCK - 1) / CVH_BLOCK); }

// bytes of a member's workspace: parent words, statistics words, then one count per workgroup
size_t cvh_cc_workspace_bytes(size_t n) { return 2 * n * sizeof(unsigned) + (size_t)cvh_cc_blocks(n) * sizeof(unsigned); }

#define CC_LAUNCH(KERNEL, GRID, ...) hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(CVH_BLOCK), 0, s, tab, nmem, ##__VA_ARGS__)

// parent[p] = root(p) of the class `mode` / `invert` name (cc_init_kernel), all unions made; the flatten launch is the caller's
static void cc_launch_forest(const CvhIoMember *tab, int nmem, unsigned grid, int mode, int invert, int conn, hipStream_t s)
{
  CC_LAUNCH(cc_init_kernel, grid, mode, invert ? 1 : 0);
  CC_LAUNCH(cc_merge_kernel, grid, conn);
}

// labels of every member into its dst (where it has one), K into its word
hipError_t cvh_launch_cc_label(const CvhIoMember *tab, int nmem, unsigned grid, int conn, int invert, bool any_labels, hipStream_t s)
{
  cc_launch_forest(tab, nmem, grid, 0, invert, conn, s);
  CC_LAUNCH(cc_flatten_count_kernel, grid);
  CC_LAUNCH(cc_scan_kernel, (unsigned)nmem);
  CC_LAUNCH(cc_number_kernel, grid);
  if (any_labels) CC_LAUNCH(cc_labels_kernel, grid);
  return hipGetLastError();
}

// cvh_measure*: the numbered forest alone, K into the member's word.  mode 0 labels the class of the level set (with `invert`), mode 1 the
// bytes of the mask in the member's dst
hipError_t cvh_launch_cc_number(const CvhIoMember *tab, int nmem, unsigned grid, int mode, int conn, int invert, hipStream_t s)
{
  cc_launch_forest(tab, nmem, grid, mode, mode == 0 ? invert : 0, conn, s);
  CC_LAUNCH(cc_flatten_count_kernel, grid);
  CC_LAUNCH(cc_scan_kernel, (unsigned)nmem);
  CC_LAUNCH(cc_number_kernel, grid);
  return hipGetLastError();
}

// behind cvh_launch_cc_label: the rows of every member's table (dst, K rows)
hipError_t cvh_launch_cc_table(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  CC_LAUNCH(cc_table_init_kernel, grid);
  CC_LAUNCH(cc_table_stats_kernel, grid);
  return hipGetLastError();
}

// the clean mask into every member's dst; the steps whose parameter is off are skipped (the caller runs io_mask_kernel where step 1 is)
hipError_t cvh_launch_cc_clean(const CvhIoMember *tab, int nmem, unsigned grid, int conn, int invert, unsigned min_area, long fill_holes,
                               int keep_largest, hipStream_t s)
{
  if (min_area > 1) {
    cc_launch_forest(tab, nmem, grid, 0, invert, conn, s);
    CC_LAUNCH(cc_flatten_area_kernel, grid, 0);
    CC_LAUNCH(cc_write_kernel, grid, 1, min_area);
  }
  if (fill_holes != 0) {
    cc_launch_forest(tab, nmem, grid, 2, 0, conn == 4 ? 8 : 4, s);
    CC_LAUNCH(cc_flatten_area_kernel, grid, 1);
    CC_LAUNCH(cc_write_kernel, grid, 2, fill_holes < 0 || fill_holes > 0x7fffffffl ? 0x7fffffffu : (unsigned)fill_holes);
  }
  if (keep_largest) {
    cc_launch_forest(tab, nmem, grid, 1, 0, conn, s);
    CC_LAUNCH(cc_flatten_area_kernel, grid, 0);
    CC_LAUNCH(cc_largest_kernel, grid);
    CC_LAUNCH(cc_write_kernel, grid, 3, 0u);
  }
  return hipGetLastError();
}
