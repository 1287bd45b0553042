/*
 * blz_devmat.hip -- the device matrix build: CSR(M) and CSR(M^T) from triplets that live on the GPU.
 *
 * The host build (csrc/host/blz_host.c, csr_from_coo_window) is a histogram with atomic counters, a prefix sum and a scatter
 * through atomic cursors that leaves the order inside a row arbitrary, "which no result depends on": every output word of a
 * product is the canonical residue of an exact integer sum.  The same three passes run here, one kernel each, for both
 * orientations at once:
 *   k_devmat_count    checks every index and value and histograms the rows and the columns (the check guards the atomic)
 *   k_scan_*          exclusive scan of rows + 1 u32 counters: tile sums, scan of the tile sums by one workgroup, add
 *   k_devmat_scatter  col_idx / val / val_hi of both CSRs through per-row cursors (atomicAdd returning the slot)
 *   k_devmat_palette  the distinct values of a slab, up to 257: an LDS hash per workgroup merged into a small global table
 *   k_devmat_pack     col_idx <- column | palette index << 24, in place
 * All atomics are atomicAdd / atomicCAS on global or LDS words; passes are ordered by kernel boundaries, never by flags.
 */
#include "blz_devmat.h"

namespace {

constexpr int TPB = 256;

template <int B> struct IdxOf;
template <> struct IdxOf<4> { using T = int32_t; };
template <> struct IdxOf<8> { using T = int64_t; };
template <int B> struct ValOf { using T = u32; };
template <> struct ValOf<8> { using T = unsigned long long; };

/* elements k .. k+3 of p: one (4-byte elements) or two (8-byte) 16-byte loads when p is 16-byte aligned (k is a multiple
 * of 4), four element loads otherwise */
template <typename T>
__device__ inline void load4(const T *p, long long k, bool vec, T &a, T &b, T &c, T &d)
{
	if (vec) {
		if constexpr (sizeof(T) == 4) {
			const uint4 q = *reinterpret_cast<const uint4 *>(p + k);
			a = (T)q.x, b = (T)q.y, c = (T)q.z, d = (T)q.w;
		} else {
			const ulonglong2 q0 = *reinterpret_cast<const ulonglong2 *>(p + k);
			const ulonglong2 q1 = *reinterpret_cast<const ulonglong2 *>(p + k + 2);
			a = (T)q0.x, b = (T)q0.y, c = (T)q1.x, d = (T)q1.y;
		}
	} else {
		a = p[k], b = p[k + 1], c = p[k + 2], d = p[k + 3];
	}
}

/* the m <= 4 elements from k on (the rest zero) */
template <typename T>
__device__ inline void load_upto4(const T *p, long long k, int m, bool vec, T e[4])
{
	if (m == 4) {
		load4(p, k, vec, e[0], e[1], e[2], e[3]);
	} else {
		e[0] = m > 0 ? p[k] : (T)0;
		e[1] = m > 1 ? p[k + 1] : (T)0;
		e[2] = m > 2 ? p[k + 2] : (T)0;
		e[3] = (T)0;
	}
}

/* vec bits: 1 = i, 2 = j, 4 = x is 16-byte aligned */
template <int IB, int VB>
__global__ __launch_bounds__(TPB) void k_devmat_count(const void *iv, const void *jv, const void *xv, long long nnz, long long nrows,
						      long long ncols, u64 p, u32 *cnt0, u32 *cnt1, unsigned long long *counts, int vec)
{
	using I = typename IdxOf<IB>::T;
	using V = typename ValOf<VB>::T;
	__shared__ unsigned int red[DEVMAT_COUNTS];
	if (threadIdx.x < DEVMAT_COUNTS)
		red[threadIdx.x] = 0;
	__syncthreads();
	const I *ip = (const I *)iv, *jp = (const I *)jv;
	const V *xp = (const V *)xv;
	unsigned int bad[DEVMAT_COUNTS] = { 0, 0, 0, 0, 0 };
	const long long quads = (nnz + 3) / 4;
	for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < quads; q += (long long)gridDim.x * TPB) {
		const long long k = q * 4;
		const int m = nnz - k < 4 ? (int)(nnz - k) : 4;
		I r[4], cidx[4];
		load_upto4(ip, k, m, (vec & 1) != 0, r);
		load_upto4(jp, k, m, (vec & 2) != 0, cidx);
		/* consecutive entries of one row (a sorted file) become one atomic */
		long long pr = -1, pc = -1;
		u32 run_r = 0, run_c = 0;
#pragma unroll
		for (int e = 0; e < 4; e++) {
			if (e >= m)
				break;
			const long long rr = (long long)r[e], cc = (long long)cidx[e];
			if ((unsigned long long)rr < (unsigned long long)nrows) {
				if (rr == pr) {
					run_r++;
				} else {
					if (run_r)
						atomicAdd(&cnt0[pr], run_r);
					pr = rr, run_r = 1;
				}
			} else {
				bad[DEVMAT_BAD_ROW]++;
			}
			if ((unsigned long long)cc < (unsigned long long)ncols) {
				if (cc == pc) {
					run_c++;
				} else {
					if (run_c)
						atomicAdd(&cnt1[pc], run_c);
					pc = cc, run_c = 1;
				}
			} else {
				bad[DEVMAT_BAD_COL]++;
			}
		}
		if (run_r)
			atomicAdd(&cnt0[pr], run_r);
		if (run_c)
			atomicAdd(&cnt1[pc], run_c);
		if constexpr (VB != 0) {
			V x[4];
			load_upto4(xp, k, m, (vec & 4) != 0, x);
#pragma unroll
			for (int e = 0; e < 4; e++) {
				if (e >= m)
					break;
				bad[DEVMAT_BAD_VAL] += (u64)x[e] >= p;
				bad[DEVMAT_NOT_ONE] += x[e] != (V)1;
				if constexpr (VB == 8)
					bad[DEVMAT_HIGH] += (x[e] >> 32) != 0;
			}
		}
	}
#pragma unroll
	for (int w = 0; w < DEVMAT_COUNTS; w++)
		if (bad[w])
			atomicAdd(&red[w], bad[w]);
	__syncthreads();
	/* one atomic per workgroup and non-zero count: none at all for valid entries that are all ones */
	if (threadIdx.x < DEVMAT_COUNTS && red[threadIdx.x])
		atomicAdd(&counts[threadIdx.x], (unsigned long long)red[threadIdx.x]);
}

/* exclusive scan of one value per thread over the workgroup; *total = the sum */
__device__ inline u32 block_excl_scan(u32 v, u32 *sh, u32 *total)
{
	const int t = threadIdx.x;
	sh[t] = v;
	__syncthreads();
	for (int d = 1; d < TPB; d <<= 1) {
		const u32 add = t >= d ? sh[t - d] : 0u;
		__syncthreads();
		sh[t] += add;
		__syncthreads();
	}
	const u32 incl = sh[t];
	*total = sh[TPB - 1];
	__syncthreads();
	return incl - v;
}

constexpr int SCAN_PER = DEVMAT_SCAN_TILE / TPB;	/* counters per thread */
static_assert(SCAN_PER * TPB == DEVMAT_SCAN_TILE && DEVMAT_SCAN_CHUNK == TPB, "scan tiles are whole workgroups");

/* sums[b] = sum of tile b */
__global__ __launch_bounds__(TPB) void k_scan_sums(const u32 *a, long long len, u32 *sums)
{
	__shared__ u32 sh[TPB];
	const long long base = (long long)blockIdx.x * DEVMAT_SCAN_TILE + (long long)threadIdx.x * SCAN_PER;
	u32 v = 0;
#pragma unroll
	for (int e = 0; e < SCAN_PER; e++)
		if (base + e < len)
			v += a[base + e];
	u32 total;
	(void)block_excl_scan(v, sh, &total);
	if (threadIdx.x == 0)
		sums[blockIdx.x] = total;
}

/* sums <- their exclusive scan: ONE workgroup, DEVMAT_SCAN_CHUNK sums per round, the carry in a register */
__global__ __launch_bounds__(TPB) void k_scan_tiles(u32 *sums, long long tiles)
{
	__shared__ u32 sh[TPB];
	u32 carry = 0;
	for (long long base = 0; base < tiles; base += DEVMAT_SCAN_CHUNK) {
		const long long at = base + threadIdx.x;
		const u32 v = at < tiles ? sums[at] : 0u;
		u32 total;
		const u32 ex = block_excl_scan(v, sh, &total);
		if (at < tiles)
			sums[at] = carry + ex;
		carry += total;
	}
}

/* tile b <- its exclusive scan + sums[b] */
__global__ __launch_bounds__(TPB) void k_scan_add(u32 *a, long long len, const u32 *sums)
{
	__shared__ u32 sh[TPB];
	const long long base = (long long)blockIdx.x * DEVMAT_SCAN_TILE + (long long)threadIdx.x * SCAN_PER;
	u32 w[SCAN_PER], v = 0;
#pragma unroll
	for (int e = 0; e < SCAN_PER; e++) {
		w[e] = base + e < len ? a[base + e] : 0u;
		v += w[e];
	}
	u32 total;
	u32 run = sums[blockIdx.x] + block_excl_scan(v, sh, &total);
#pragma unroll
	for (int e = 0; e < SCAN_PER; e++) {
		if (base + e < len)
			a[base + e] = run;
		run += w[e];
	}
}

template <int IB, int VB>
__global__ __launch_bounds__(TPB) void k_devmat_scatter(const void *iv, const void *jv, const void *xv, long long nnz, long long nrows,
							long long ncols, u32 *cur0, u32 *cur1, int *col0, u32 *val0, u32 *hi0, int *col1,
							u32 *val1, u32 *hi1, int vec)
{
	using I = typename IdxOf<IB>::T;
	using V = typename ValOf<VB>::T;
	const I *ip = (const I *)iv, *jp = (const I *)jv;
	const V *xp = (const V *)xv;
	const long long quads = (nnz + 3) / 4;
	for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < quads; q += (long long)gridDim.x * TPB) {
		const long long k = q * 4;
		const int m = nnz - k < 4 ? (int)(nnz - k) : 4;
		I r[4], cidx[4];
		V x[4] = { 0, 0, 0, 0 };
		load_upto4(ip, k, m, (vec & 1) != 0, r);
		load_upto4(jp, k, m, (vec & 2) != 0, cidx);
		if constexpr (VB != 0)
			load_upto4(xp, k, m, (vec & 4) != 0, x);
#pragma unroll
		for (int e = 0; e < 4; e++) {
			if (e >= m)
				break;
			const long long rr = (long long)r[e], cc = (long long)cidx[e];
			if ((unsigned long long)rr >= (unsigned long long)nrows || (unsigned long long)cc >= (unsigned long long)ncols)
				continue;
			const u32 lo = (u32)x[e];
			u32 hi = 0;
			if constexpr (VB == 8)
				hi = (u32)(x[e] >> 32);
			const u32 s0 = atomicAdd(&cur0[rr], 1u);
			if ((long long)s0 < nnz) {
				col0[s0] = (int)cc;
				if (val0)
					val0[s0] = lo;
				if (hi0)
					hi0[s0] = hi;
			}
			const u32 s1 = atomicAdd(&cur1[cc], 1u);
			if ((long long)s1 < nnz) {
				col1[s1] = (int)rr;
				if (val1)
					val1[s1] = lo;
				if (hi1)
					hi1[s1] = hi;
			}
		}
	}
}

__device__ inline u32 pal_hash(unsigned long long key)
{
	const u32 v = (u32)key, vh = (u32)(key >> 32);
	return (((v ^ vh * 0x9E3779B1u) * 2654435761u) >> 20) & (DEVMAT_PAL_SLOTS - 1);
}

/* key into an open-addressing table of DEVMAT_PAL_SLOTS words; 1: it was new, 0: it was there, -1: no room */
__device__ inline int pal_insert(unsigned long long *table, unsigned long long key)
{
	u32 h = pal_hash(key);
	for (int probe = 0; probe < DEVMAT_PAL_SLOTS; probe++) {
		const unsigned long long old = atomicCAS(&table[h], DEVMAT_PAL_EMPTY, key);
		if (old == DEVMAT_PAL_EMPTY)
			return 1;
		if (old == key)
			return 0;
		h = (h + 1) & (DEVMAT_PAL_SLOTS - 1);
	}
	return -1;
}

/* the same on the global table, reading before it swaps: a value that is there already costs no atomic */
__device__ inline int pal_insert_global(unsigned long long *table, unsigned long long key)
{
	u32 h = pal_hash(key);
	for (int probe = 0; probe < DEVMAT_PAL_SLOTS; probe++) {
		unsigned long long old = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (old == DEVMAT_PAL_EMPTY)
			old = atomicCAS(&table[h], DEVMAT_PAL_EMPTY, key);
		if (old == DEVMAT_PAL_EMPTY)
			return 1;
		if (old == key)
			return 0;
		h = (h + 1) & (DEVMAT_PAL_SLOTS - 1);
	}
	return -1;
}

enum { PAL_OVER = 4 * DEVMAT_PAL_SLOTS };	/* added to *count by a workgroup that saw too many values */

template <bool WIDE>
__global__ __launch_bounds__(TPB) void k_devmat_palette(const u32 *val, const u32 *hi, long long nnz, unsigned long long *table,
							unsigned int *count)
{
	__shared__ unsigned long long lds[DEVMAT_PAL_SLOTS];
	__shared__ unsigned int lcount, gcount;
	for (int s = threadIdx.x; s < DEVMAT_PAL_SLOTS; s += TPB)
		lds[s] = DEVMAT_PAL_EMPTY;
	if (threadIdx.x == 0) {
		lcount = 0;
		gcount = __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__syncthreads();
	if (gcount > DEVMAT_PAL_MAX)	/* somebody has seen too many already */
		return;
	/* every thread looks at the count before each insertion and TPB threads insert at a time: the table never holds more
	 * than DEVMAT_PAL_MAX + 1 + TPB keys, half its slots */
	unsigned long long last = DEVMAT_PAL_EMPTY;
	for (long long k = (long long)blockIdx.x * TPB + threadIdx.x; k < nnz; k += (long long)gridDim.x * TPB) {
		unsigned long long key = val[k];
		if constexpr (WIDE)
			key |= (unsigned long long)hi[k] << 32;
		if (key == last)
			continue;
		last = key;
		if (*(volatile unsigned int *)&lcount > DEVMAT_PAL_MAX)
			break;
		if (pal_insert(lds, key) != 0)
			atomicAdd(&lcount, 1u);
	}
	__syncthreads();
	if (lcount > DEVMAT_PAL_MAX) {
		if (threadIdx.x == 0)
			atomicAdd(count, (unsigned int)PAL_OVER);
		return;
	}
	for (int s = threadIdx.x; s < DEVMAT_PAL_SLOTS; s += TPB) {
		const unsigned long long key = lds[s];
		if (key == DEVMAT_PAL_EMPTY)
			continue;
		if (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > DEVMAT_PAL_MAX)
			break;
		const int rc = pal_insert_global(table, key);
		if (rc != 0)
			atomicAdd(count, rc > 0 ? 1u : (unsigned int)PAL_OVER);
	}
}

/* keys[0 .. min(*count, DEVMAT_PAL_MAX)) <- the keys of the table, one workgroup */
__global__ __launch_bounds__(TPB) void k_devmat_palette_keys(const unsigned long long *table, unsigned long long *keys)
{
	__shared__ unsigned int at;
	if (threadIdx.x == 0)
		at = 0;
	__syncthreads();
	for (int s = threadIdx.x; s < DEVMAT_PAL_SLOTS; s += TPB) {
		const unsigned long long key = table[s];
		if (key == DEVMAT_PAL_EMPTY)
			continue;
		const unsigned int idx = atomicAdd(&at, 1u);
		if (idx < DEVMAT_PAL_MAX)
			keys[idx] = key;
	}
}

template <bool WIDE>
__global__ __launch_bounds__(TPB) void k_devmat_pack(int *col, const u32 *val, const u32 *hi, long long nnz,
						     const unsigned long long *keys, int nkeys)
{
	__shared__ unsigned long long sk[DEVMAT_PAL_MAX];
	for (int s = threadIdx.x; s < DEVMAT_PAL_MAX; s += TPB)
		sk[s] = s < nkeys ? keys[s] : DEVMAT_PAL_EMPTY;
	__syncthreads();
	auto index_of = [&](unsigned long long key) -> u32 {
		int lo = 0, hi_ = nkeys - 1;	/* the key is there: the palette was made from these values */
		while (lo < hi_) {
			const int mid = (lo + hi_) >> 1;
			if (sk[mid] < key)
				lo = mid + 1;
			else
				hi_ = mid;
		}
		return (u32)lo;
	};
	/* col, val and hi come from hipMalloc: 16-byte accesses on whole quads, the last entries one by one */
	const long long quads = nnz / 4;
	for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < quads; q += (long long)gridDim.x * TPB) {
		uint4 cq = *reinterpret_cast<const uint4 *>(col + q * 4);
		const uint4 vq = *reinterpret_cast<const uint4 *>(val + q * 4);
		uint4 hq = make_uint4(0, 0, 0, 0);
		if constexpr (WIDE)
			hq = *reinterpret_cast<const uint4 *>(hi + q * 4);
		cq.x |= index_of(vq.x | (unsigned long long)hq.x << 32) << 24;
		cq.y |= index_of(vq.y | (unsigned long long)hq.y << 32) << 24;
		cq.z |= index_of(vq.z | (unsigned long long)hq.z << 32) << 24;
		cq.w |= index_of(vq.w | (unsigned long long)hq.w << 32) << 24;
		*reinterpret_cast<uint4 *>(col + q * 4) = cq;
	}
	if (blockIdx.x == 0) {
		const long long k = quads * 4 + threadIdx.x;
		if (k < nnz) {
			unsigned long long key = val[k];
			if constexpr (WIDE)
				key |= (unsigned long long)hi[k] << 32;
			col[k] = (int)((u32)col[k] | index_of(key) << 24);
		}
	}
}

inline int grid_for(const KernelCfg &c, long long items)
{
	const long long want = (items + TPB - 1) / TPB, cap = (long long)(c.num_cu > 0 ? c.num_cu : 256) * 8;
	return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

inline int vec_bits(const void *i, const void *j, const void *x)
{
	return (((uintptr_t)i & 15) == 0 ? 1 : 0) | (((uintptr_t)j & 15) == 0 ? 2 : 0) | (((uintptr_t)x & 15) == 0 ? 4 : 0);
}

}  // namespace

/* every (idx_bytes, val_bytes) pair of blz_set_matrix_device: DEVMAT_INSTANCES(X) expands X(IB, VB) for each */
#define DEVMAT_INSTANCES(X) X(4, 0) X(4, 4) X(4, 8) X(8, 0) X(8, 4) X(8, 8)

hipError_t launch_devmat_count(const KernelCfg &c, int idx_bytes, int val_bytes, const void *i, const void *j, const void *x,
			       long long nnz, long long nrows, long long ncols, u32 *cnt0, u32 *cnt1, unsigned long long *counts,
			       hipStream_t s)
{
	if (nnz <= 0)
		return hipSuccess;
	const int grid = grid_for(c, (nnz + 3) / 4), vec = vec_bits(i, j, x);
#define X(IB, VB)                                                                                                          \
	if (idx_bytes == IB && val_bytes == VB) {                                                                          \
		k_devmat_count<IB, VB><<<grid, TPB, 0, s>>>(i, j, x, nnz, nrows, ncols, c.m.p, cnt0, cnt1, counts, vec);     \
		return hipGetLastError();                                                                                  \
	}
	DEVMAT_INSTANCES(X)
#undef X
	return hipErrorInvalidValue;
}

long long devmat_scan_tiles(long long len) { return len > 0 ? (len + DEVMAT_SCAN_TILE - 1) / DEVMAT_SCAN_TILE : 0; }

hipError_t launch_devmat_scan(u32 *a, long long len, u32 *sums, hipStream_t s)
{
	const long long tiles = devmat_scan_tiles(len);
	if (tiles <= 0)
		return hipSuccess;
	k_scan_sums<<<(unsigned)tiles, TPB, 0, s>>>(a, len, sums);
	k_scan_tiles<<<1, TPB, 0, s>>>(sums, tiles);
	k_scan_add<<<(unsigned)tiles, TPB, 0, s>>>(a, len, sums);
	return hipGetLastError();
}

hipError_t launch_devmat_scatter(const KernelCfg &c, int idx_bytes, int val_bytes, const void *i, const void *j, const void *x,
				 long long nnz, long long nrows, long long ncols, u32 *cur0, u32 *cur1, int *col0, u32 *val0, u32 *hi0,
				 int *col1, u32 *val1, u32 *hi1, hipStream_t s)
{
	if (nnz <= 0)
		return hipSuccess;
	const int grid = grid_for(c, (nnz + 3) / 4), vec = vec_bits(i, j, x);
#define X(IB, VB)                                                                                                          \
	if (idx_bytes == IB && val_bytes == VB) {                                                                          \
		k_devmat_scatter<IB, VB><<<grid, TPB, 0, s>>>(i, j, x, nnz, nrows, ncols, cur0, cur1, col0, val0, hi0, col1, \
							       val1, hi1, vec);                                              \
		return hipGetLastError();                                                                                  \
	}
	DEVMAT_INSTANCES(X)
#undef X
	return hipErrorInvalidValue;
}

hipError_t launch_devmat_palette(const KernelCfg &c, const u32 *val, const u32 *hi, long long nnz, unsigned long long *table,
				 unsigned int *count, unsigned long long *keys, hipStream_t s)
{
	if (nnz > 0) {
		const int grid = grid_for(c, (nnz + 3) / 4);
		if (hi)
			k_devmat_palette<true><<<grid, TPB, 0, s>>>(val, hi, nnz, table, count);
		else
			k_devmat_palette<false><<<grid, TPB, 0, s>>>(val, hi, nnz, table, count);
	}
	k_devmat_palette_keys<<<1, TPB, 0, s>>>(table, keys);
	return hipGetLastError();
}

hipError_t launch_devmat_pack(const KernelCfg &c, int *col, const u32 *val, const u32 *hi, long long nnz,
			      const unsigned long long *keys, int nkeys, hipStream_t s)
{
	if (nnz <= 0 || nkeys < 1)
		return hipSuccess;
	const int grid = grid_for(c, (nnz + 3) / 4);
	if (hi)
		k_devmat_pack<true><<<grid, TPB, 0, s>>>(col, val, hi, nnz, keys, nkeys);
	else
		k_devmat_pack<false><<<grid, TPB, 0, s>>>(col, val, hi, nnz, keys, nkeys);
	return hipGetLastError();
}
