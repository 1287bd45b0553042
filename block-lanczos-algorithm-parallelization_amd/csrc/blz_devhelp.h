/* blz_devhelp.h -- the few helpers the device-block kernel files share (blz_devalg.hip, blz_devw32.hip, blz_devsmall.hip,
 * blz_devmfma.hip, blz_devrhs.hip).  C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVHELP_H
#define BLZ_DEVHELP_H

#include <atomic>

#include "blz_kernels.h"

__device__ __forceinline__ u64 shfl64(u64 v, int src)
{
	return (u64)__shfl((unsigned long long)v, src, 64);
}

inline int log2_ceil(int v)
{
	int lg = 0;
	while ((1 << lg) < v)
		lg++;
	return lg;
}

/* Above 48 KB of dynamic LDS a kernel must be told its limit.  K is the kernel instantiation, `most` the most bytes it can ask
 * for: it is told once per instantiation and device, and a failure is the launcher's error. */
template <auto K>
hipError_t dev_lds_limit(size_t lds, size_t most)
{
	constexpr int MAX_DEVICES = 64;
	static std::atomic<bool> told[MAX_DEVICES];
	if (lds <= 48 * 1024)
		return hipSuccess;
	int dev = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess)
		return e;
	const bool known = dev >= 0 && dev < MAX_DEVICES;
	if (known && told[dev].load())
		return hipSuccess;
	e = hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
	if (e == hipSuccess && known)
		told[dev].store(true);
	return e;
}

#endif
