/*
 * blz_devorder.hip -- the device renumbering: blz_reorder's order made on the GPU, before the device
 * matrix build (blz_devmat.hip) runs on the relabelled triplets.
 *
 * blz_reorder (csrc/host/blz_host.c) is an atomic minimum per entry and a stable counting sort, twice: rows by their smallest
 * column, then columns by their smallest NEW row; rows / columns without entries take the key ncols / nrows and so come
 * last; ties stay in ascending original index.  A minimum does not depend on the order of its operands and a stable sort has
 * one answer, so the numbering made here is the host's word for word although no two runs schedule alike:
 *   k_devorder_fill     key[] <- the key of an index without entries
 *   k_devorder_min      key[i] <- min(key[i], j), or key[j] <- min(key[j], perm[i]); both indices checked before either is used
 *   k_devorder_digits   per tile of DEVORDER_SORT_TILE items: how many carry each value of the current digit (digit-major)
 *   (launch_devmat_scan over the count matrix: where every (digit, tile) group starts)
 *   k_devorder_scatter  item -> start of its (digit, tile) group + the number of EARLIER items of the tile with that digit,
 *                       counted from an LDS copy of the tile's digits by a plain loop: stable by construction
 *   k_devorder_relabel  ni = row_perm[i], nj = col_perm[j] as int32, -1 for an index outside the matrix
 * The only atomics are atomicMin on global keys and atomicAdd on an LDS histogram; no workgroup waits for another.
 */
#include "blz_devorder.h"
#include "blz_devmat.h"

namespace {

constexpr int TPB = 256;
static_assert(DEVORDER_SORT_TILE == TPB && DEVORDER_DIGITS == TPB, "one item and one digit value per thread of a workgroup");

template <int B> struct IdxOf;
template <> struct IdxOf<4> { using T = int32_t; };
template <> struct IdxOf<8> { using T = int64_t; };

/* the m <= 4 elements from k on (the rest zero): one (4-byte elements) or two (8-byte) 16-byte loads for a whole quad when p is
 * 16-byte aligned (k is a multiple of 4), element loads otherwise */
template <typename T>
__device__ inline void load_upto4(const T *p, long long k, int m, bool vec, T e[4])
{
	if (m == 4 && vec) {
		if constexpr (sizeof(T) == 4) {
			const uint4 q = *reinterpret_cast<const uint4 *>(p + k);
			e[0] = (T)q.x, e[1] = (T)q.y, e[2] = (T)q.z, e[3] = (T)q.w;
		} else {
			const ulonglong2 q0 = *reinterpret_cast<const ulonglong2 *>(p + k);
			const ulonglong2 q1 = *reinterpret_cast<const ulonglong2 *>(p + k + 2);
			e[0] = (T)q0.x, e[1] = (T)q0.y, e[2] = (T)q1.x, e[3] = (T)q1.y;
		}
	} else {
		e[0] = m > 0 ? p[k] : (T)0;
		e[1] = m > 1 ? p[k + 1] : (T)0;
		e[2] = m > 2 ? p[k + 2] : (T)0;
		e[3] = m > 3 ? p[k + 3] : (T)0;
	}
}

__global__ __launch_bounds__(TPB) void k_devorder_fill(int32_t *key, long long count, int32_t value)
{
	for (long long k = (long long)blockIdx.x * TPB + threadIdx.x; k < count; k += (long long)gridDim.x * TPB)
		key[k] = value;
}

/* perm[k] <- k: the order of keys that are all zero */
__global__ __launch_bounds__(TPB) void k_devorder_iota(int32_t *perm, long long count)
{
	for (long long k = (long long)blockIdx.x * TPB + threadIdx.x; k < count; k += (long long)gridDim.x * TPB)
		perm[k] = (int32_t)k;
}

/* vec bits: 1 = i, 2 = j is 16-byte aligned */
template <int IB, bool BYCOL>
__global__ __launch_bounds__(TPB) void k_devorder_min(const void *iv, const void *jv, long long nnz, long long nrows, long long ncols,
						      const int32_t *perm, int32_t *key, int vec)
{
	using I = typename IdxOf<IB>::T;
	const I *ip = (const I *)iv, *jp = (const I *)jv;
	const long long quads = (nnz + 3) / 4;
	for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < quads; q += (long long)gridDim.x * TPB) {
		const long long k = q * 4;
		const int m = nnz - k < 4 ? (int)(nnz - k) : 4;
		I r[4], cidx[4];
		load_upto4(ip, k, m, (vec & 1) != 0, r);
		load_upto4(jp, k, m, (vec & 2) != 0, cidx);
		/* consecutive entries with one target (the rows of a sorted file) become one atomic */
		long long at = -1;
		int32_t least = 0;
#pragma unroll
		for (int e = 0; e < 4; e++) {
			if (e >= m)
				break;
			const long long rr = (long long)r[e], cc = (long long)cidx[e];
			if ((unsigned long long)rr >= (unsigned long long)nrows || (unsigned long long)cc >= (unsigned long long)ncols)
				continue;
			const long long target = BYCOL ? cc : rr;
			const int32_t v = BYCOL ? perm[rr] : (int32_t)cc;
			if (target == at) {
				least = v < least ? v : least;
			} else {
				if (at >= 0)
					atomicMin(&key[at], least);
				at = target, least = v;
			}
		}
		if (at >= 0)
			atomicMin(&key[at], least);
	}
}

/* counters[d * tiles + b] = items of tile b whose digit is d */
__global__ __launch_bounds__(TPB) void k_devorder_digits(const int32_t *key, long long count, int shift, long long tiles, u32 *counters)
{
	__shared__ unsigned int hist[DEVORDER_DIGITS];
	hist[threadIdx.x] = 0;
	__syncthreads();
	const long long at = (long long)blockIdx.x * DEVORDER_SORT_TILE + threadIdx.x;
	if (at < count)
		atomicAdd(&hist[((u32)key[at] >> shift) & (DEVORDER_DIGITS - 1)], 1u);
	__syncthreads();
	counters[(long long)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

/* starts: the exclusive scan of k_devorder_digits' matrix.  The item at place `at` of the pass's input (item[at], or `at` itself
 * on the first pass, item == NULL) goes to place starts[digit * tiles + tile] + its rank among the tile's items of that digit.
 * perm == NULL: key_out / item_out take it there; perm != NULL (the last pass): perm[item] = place. */
__global__ __launch_bounds__(TPB) void k_devorder_scatter(const int32_t *key, const int32_t *item, long long count, int shift,
							  long long tiles, const u32 *starts, int32_t *key_out, int32_t *item_out,
							  int32_t *perm)
{
	__shared__ unsigned short dig[DEVORDER_SORT_TILE];
	const int t = threadIdx.x;
	const long long at = (long long)blockIdx.x * DEVORDER_SORT_TILE + t;
	const bool have = at < count;
	const int32_t kv = have ? key[at] : 0;
	const unsigned short d = have ? (unsigned short)(((u32)kv >> shift) & (DEVORDER_DIGITS - 1)) : (unsigned short)DEVORDER_DIGITS;
	dig[t] = d;
	__syncthreads();
	if (!have)
		return;
	u32 rank = 0;
	for (int e = 0; e < t; e++)
		rank += dig[e] == d;
	const long long place = (long long)starts[(long long)d * tiles + blockIdx.x] + rank;
	const long long id = item ? (long long)item[at] : at;
	if (place >= count || (unsigned long long)id >= (unsigned long long)count)	/* (never, on counters this pass made) */
		return;
	if (perm) {
		perm[id] = (int32_t)place;
	} else {
		key_out[place] = kv;
		item_out[place] = (int32_t)id;
	}
}

template <int IB>
__global__ __launch_bounds__(TPB) void k_devorder_relabel(const void *iv, const void *jv, long long nnz, long long nrows, long long ncols,
							  const int32_t *row_perm, const int32_t *col_perm, int32_t *ni, int32_t *nj, int vec)
{
	using I = typename IdxOf<IB>::T;
	const I *ip = (const I *)iv, *jp = (const I *)jv;
	const long long quads = (nnz + 3) / 4;
	for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < quads; q += (long long)gridDim.x * TPB) {
		const long long k = q * 4;
		const int m = nnz - k < 4 ? (int)(nnz - k) : 4;
		I r[4], cidx[4];
		load_upto4(ip, k, m, (vec & 1) != 0, r);
		load_upto4(jp, k, m, (vec & 2) != 0, cidx);
		int32_t a[4], b[4];
#pragma unroll
		for (int e = 0; e < 4; e++) {
			const long long rr = (long long)r[e], cc = (long long)cidx[e];
			a[e] = e < m && (unsigned long long)rr < (unsigned long long)nrows ? row_perm[rr] : -1;
			b[e] = e < m && (unsigned long long)cc < (unsigned long long)ncols ? col_perm[cc] : -1;
		}
		if (m == 4) {		/* ni, nj come from hipMalloc and k is a multiple of 4 */
			*reinterpret_cast<int4 *>(ni + k) = make_int4(a[0], a[1], a[2], a[3]);
			*reinterpret_cast<int4 *>(nj + k) = make_int4(b[0], b[1], b[2], b[3]);
		} else {
			for (int e = 0; e < m; e++)
				ni[k + e] = a[e], nj[k + e] = b[e];
		}
	}
}

inline int grid_for(const KernelCfg &c, long long items)
{
	const long long want = (items + TPB - 1) / TPB, cap = (long long)(c.num_cu > 0 ? c.num_cu : 256) * 8;
	return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

inline int vec_bits(const void *i, const void *j)
{
	return (((uintptr_t)i & 15) == 0 ? 1 : 0) | (((uintptr_t)j & 15) == 0 ? 2 : 0);
}

}  // namespace

hipError_t launch_devorder_fill(const KernelCfg &c, int32_t *key, long long count, int32_t value, hipStream_t s)
{
	if (count <= 0)
		return hipSuccess;
	k_devorder_fill<<<grid_for(c, count), TPB, 0, s>>>(key, count, value);
	return hipGetLastError();
}

hipError_t launch_devorder_min(const KernelCfg &c, int idx_bytes, const void *i, const void *j, long long nnz, long long nrows,
			       long long ncols, const int32_t *perm, int32_t *key, int by_col, hipStream_t s)
{
	if (nnz <= 0)
		return hipSuccess;
	if ((idx_bytes != 4 && idx_bytes != 8) || (by_col && !perm))
		return hipErrorInvalidValue;
	const int grid = grid_for(c, (nnz + 3) / 4), vec = vec_bits(i, j);
	if (idx_bytes == 4 && !by_col)
		k_devorder_min<4, false><<<grid, TPB, 0, s>>>(i, j, nnz, nrows, ncols, perm, key, vec);
	else if (idx_bytes == 4)
		k_devorder_min<4, true><<<grid, TPB, 0, s>>>(i, j, nnz, nrows, ncols, perm, key, vec);
	else if (!by_col)
		k_devorder_min<8, false><<<grid, TPB, 0, s>>>(i, j, nnz, nrows, ncols, perm, key, vec);
	else
		k_devorder_min<8, true><<<grid, TPB, 0, s>>>(i, j, nnz, nrows, ncols, perm, key, vec);
	return hipGetLastError();
}

int devorder_sort_passes(long long nkeys)
{
	int bits = 0;
	while (bits < 63 && (nkeys >> bits) != 0)
		bits++;
	return (bits + DEVORDER_DIGIT_BITS - 1) / DEVORDER_DIGIT_BITS;
}

long long devorder_sort_tiles(long long count) { return count > 0 ? (count + DEVORDER_SORT_TILE - 1) / DEVORDER_SORT_TILE : 0; }
long long devorder_sort_counters(long long count) { return devorder_sort_tiles(count) * DEVORDER_DIGITS; }

hipError_t launch_devorder_sort(const KernelCfg &c, const int32_t *key, long long count, long long nkeys, int32_t *perm,
				int32_t *const buf_key[2], int32_t *const buf_item[2], u32 *counters, u32 *sums, hipStream_t s)
{
	if (count <= 0)
		return hipSuccess;
	const int passes = devorder_sort_passes(nkeys);
	if (passes == 0) {	/* every key is 0 */
		k_devorder_iota<<<grid_for(c, count), TPB, 0, s>>>(perm, count);
		return hipGetLastError();
	}
	const long long tiles = devorder_sort_tiles(count);
	const int32_t *kin = key, *iin = nullptr;
	for (int q = 0; q < passes; q++) {
		const bool last = q == passes - 1;
		const int shift = q * DEVORDER_DIGIT_BITS;
		k_devorder_digits<<<(unsigned)tiles, TPB, 0, s>>>(kin, count, shift, tiles, counters);
		hipError_t e = hipGetLastError();
		if (e == hipSuccess)
			e = launch_devmat_scan(counters, devorder_sort_counters(count), sums, s);
		if (e != hipSuccess)
			return e;
		k_devorder_scatter<<<(unsigned)tiles, TPB, 0, s>>>(kin, iin, count, shift, tiles, counters, last ? nullptr : buf_key[q & 1],
								  last ? nullptr : buf_item[q & 1], last ? perm : nullptr);
		if ((e = hipGetLastError()) != hipSuccess)
			return e;
		kin = buf_key[q & 1], iin = buf_item[q & 1];
	}
	return hipSuccess;
}

hipError_t launch_devorder_relabel(const KernelCfg &c, int idx_bytes, const void *i, const void *j, long long nnz,
				   long long nrows, long long ncols, const int32_t *row_perm, const int32_t *col_perm, int32_t *ni,
				   int32_t *nj, hipStream_t s)
{
	if (nnz <= 0)
		return hipSuccess;
	const int grid = grid_for(c, (nnz + 3) / 4), vec = vec_bits(i, j);
	if (idx_bytes == 4)
		k_devorder_relabel<4><<<grid, TPB, 0, s>>>(i, j, nnz, nrows, ncols, row_perm, col_perm, ni, nj, vec);
	else if (idx_bytes == 8)
		k_devorder_relabel<8><<<grid, TPB, 0, s>>>(i, j, nnz, nrows, ncols, row_perm, col_perm, ni, nj, vec);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}
