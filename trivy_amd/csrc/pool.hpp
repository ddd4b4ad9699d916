// The process-wide pool of worker threads (pool.cpp): plan construction, the resolver, the
// layer walk and the device pipeline's host stages all run their parallel loops on it.
#pragma once
#include <cstddef>
#include <functional>

namespace tsg {

// f(i) for i in [0, n) on the caller and up to nthreads - 1 pool workers, `grain` indices a
// claim; serial when nthreads <= 1 or n < 2 * grain
void pool_for(size_t n, int nthreads, const std::function<void(size_t)>& f, size_t grain = 64);
// the pool holds at least this many worker threads
void pool_reserve(int threads);

}  // namespace tsg
