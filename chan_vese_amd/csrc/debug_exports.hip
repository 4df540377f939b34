// debug_exports.hip — diagnostic exports that include/chanvese_hip.h does not declare (the tests and tools/ bind them by name).
#include "cvh_host.h"

// Diagnostic (not part of include/chanvese_hip.h): the strip table for a geometry, without a device.  out needs S + 1 ints.
extern "C" int cvh_debug_strip_bounds(int kind, int h, int tiles_x, int S, int strip_rows, int nblocks, int cls, int cskew, int skew, int *out)
{
  if (!out || S < 1 || h < 1 || (kind != 2 && kind != 3)) return CVH_ERR_ARG;
  std::vector<int> b;
  compute_strip_bounds(kind, h, tiles_x, S, strip_rows, nblocks, cls, cskew, skew, b);
  memcpy(out, b.data(), b.size() * sizeof(int));
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): which per-launch data flow resolve_geometry() picks for a shape and option set, without a
// device -- 0 tile kernel, 2 wave kernel, 3 wave kernel with 2 pixels per lane -- and its grid (tests/test_host_geometry.py pins the dispatch,
// e.g. the tile kernel from 2^28 pixels on, which no GPU test launches).
extern "C" int cvh_debug_data_flow(int h, int w, int channels, int math_mode, int kernel, int state_bits, int num_cus, int *flow, int *tiles_x,
                                   int *tiles_y, int *strip_rows)
{
  if (h < 1 || w < 1 || (channels != 1 && channels != 3) || !flow) return CVH_ERR_ARG;
  cvh_context c;
  c.h = h; c.w = w; c.C = channels; c.n = (size_t)h * (size_t)w;
  c.math_mode = math_mode; c.kernel = kernel; c.state_bits = state_bits; c.num_cus = num_cus > 0 ? num_cus : 256;
  const Geometry g = resolve_geometry(&c);
  *flow = g.strip;
  if (tiles_x) *tiles_x = g.tiles_x;
  if (tiles_y) *tiles_y = g.tiles_y;
  if (strip_rows) *strip_rows = g.strip_rows;
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): the synchronisation words of the last resident launch: {error, 0, generation of
// the arrival line of tile 0 .. n-1, generation of the release line of tile 0 .. n-1}.
extern "C" int cvh_debug_resident_read(cvh_context *c, unsigned *out, int ngo)
{
  if (!c || !out || ngo < 0 || ngo > CVH_RESIDENT_MAX_TILES) return CVH_ERR_ARG;
  if (!c->d_resident) return fail(c, CVH_ERR_STATE, "no resident launch yet");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned> tmp(sizeof(CvhResident) / sizeof(unsigned));
  HIPCHK(c, hipMemcpy(tmp.data(), c->d_resident, sizeof(CvhResident), hipMemcpyDeviceToHost));
  out[0] = tmp[0]; out[1] = tmp[1] | (tmp[2] << 12) | (tmp[3] << 24);   // error; t_first | nit << 12 | steps_done as the kernel read it << 24
  for (int i = 0; i < ngo; ++i) { out[2 + i] = tmp[16 + (size_t)i * 16]; out[2 + ngo + i] = tmp[16 + (size_t)CVH_RESIDENT_MAX_TILES * 16 + (size_t)i * 16]; }
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): the CUs of the context's device, what the automatic geometry and a fused batch's
// shares are sized for (tests/test_gpu_fused_batch_matrix.py recomputes a member's share geometry from it).
extern "C" int cvh_debug_num_cus(cvh_context *c, int *out)
{
  if (!c || !out) return CVH_ERR_ARG;
  *out = c->num_cus;
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): copies the stamp buffer of "debug_times".
extern "C" int cvh_debug_read(cvh_context *c, unsigned long long *out, long max_words, long *words, int *nblocks)
{
  if (!c || !out || !words) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  long n = (long)c->dbg_words < max_words ? (long)c->dbg_words : max_words;
  *words = n;
  if (nblocks) *nblocks = c->last_nparts > 0 ? c->last_nparts : resolve_geometry(c).nblocks;   // the grid the stamps belong to (a fused batch's share)
  if (n > 0 && c->d_dbg) HIPCHK(c, hipMemcpy(out, c->d_dbg, (size_t)n * 8, hipMemcpyDeviceToHost));
  return CVH_OK;
}
