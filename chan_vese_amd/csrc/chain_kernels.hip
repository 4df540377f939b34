// chain_kernels.hip — the flush kernel of chain mode (chain_device.h): at a host synchronisation point the last launch's
// iteration has no successor to book it.  One workgroup books it (norm, stop rule, trace row) and writes the region
// means of the current level set into the state block (cvh_get_means, kernels that read c1/c2 from there).
#include "chain_device.h"

using namespace cvh_dev;

namespace {

template <int C>
__global__ __launch_bounds__(CVH_BLOCK) void csv_chain_flush_kernel(const CvhStepArgs a)
{
  __shared__ double sred[4];
  const int lane = threadIdx.x & 63;
  // sums of the level set after the last BOOKED iteration live in set (pb + steps_done); a stop found now leaves it there
  const int done = chain_bookkeeping<C>(a, true, nullptr, nullptr, sred);
  const long long entry = a.chain->v[(a.chain_pb + done) & 3][lane];
  double c1[C], c2[C];
  chain_means<C>(a, entry, c1, c2);
  // A NaN norm in row t - 1: iteration t - 1 left a NaN in the level set, whose means (row t) are NaN in the reference -- H_eps(NaN)
  // makes every sum NaN -- while the FAST H_eps clamps a NaN argument into a finite value and the fixed-point sums stay finite.  The
  // rows are mended here, where the host is about to read them (the step kernels' bookkeeper stays as it is).
  if (a.trace) {
    constexpr int TR = 2 * C + 1;
    const int rows = done < a.trace_cap ? done : a.trace_cap;
    for (int t = 1 + (int)threadIdx.x; t < rows; t += CVH_BLOCK) {
      const double prev = a.trace[(size_t)(t - 1) * TR + 2 * C];
      if (prev != prev)
        for (int k = 0; k < 2 * C; ++k) a.trace[(size_t)t * TR + k] = prev;
    }
  }
  if (threadIdx.x == 0) {
    const double nrm = a.st->norm;
    const bool went_nan = done > 0 && nrm != nrm;   // the last booked iteration left a NaN in the level set: its means are NaN (finalize(), csv_device.h)
#pragma unroll
    for (int k = 0; k < C; ++k) { a.st->c1[k] = went_nan ? nrm : c1[k]; a.st->c2[k] = went_nan ? nrm : c2[k]; }
    // what cvh_sync reports, straight into the pinned host block {steps_done, stopped, norm}: no device-to-host copy behind the flush
    if (a.host_status) {
      const long long nb = __double_as_longlong(a.st->norm);
      __hip_atomic_store(&a.host_status[2], (int)nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&a.host_status[3], (int)(nb >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&a.host_status[1], a.st->stopped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&a.host_status[0], a.st->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace

hipError_t cvh_launch_chain_flush(const CvhStepArgs &a, int channels, hipStream_t s)
{
  if (channels == 1) hipLaunchKernelGGL(csv_chain_flush_kernel<1>, dim3(1), dim3(CVH_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(csv_chain_flush_kernel<3>, dim3(1), dim3(CVH_BLOCK), 0, s, a);
  return hipGetLastError();
}
