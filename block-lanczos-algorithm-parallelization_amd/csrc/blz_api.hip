/*
 * blz_api.hip -- the device half of the C ABI declared in include/blz.h: contexts, HBM residency,
 * kernel sequencing, HIP-event timing and the RCCL exchange steps.
 *
 * HBM layout per context (one per GPU).  "side 0" = rows of v/Av/p, "side 1" = rows of tmp.
 *   slab[V], slab[AV], slab[P] : this rank's rows of side 0, slab[TMP] : its rows of side 1, row-major
 *   rows x n, padded to `stride` rows.  With one rank these ARE the reference's N x n arrays.
 *   gath[side] (only with nranks > 1): the all-gathered operand of a product, K = ag_chunks pieces:
 *   [piece k][rank g][stride/K rows][n] -- ncclAllGather number k moves piece k of every slab and lands
 *   contiguously, so the product on csr[t][k] (the entries whose columns lie in piece k) can run on the compute
 *   stream while piece k+1 is still in flight on the exchange stream.
 *   csr[0][k] / csr[1][k] = this rank's rows of M / M^T restricted to the columns of piece k.
 *   small  = [vtAv | vtAAv | winv | d | c | vtAvd], 6*n*n words;  ctl = DevCtl.
 *   slab[4 + side] (one rank, allocated on first use): the scratch slabs blz_apply_device multiplies in, never a caller's block.
 *   devalg_partial (allocated on first use): the partial rows of blz_dot_device, never the `partial` of an iteration in flight.
 *   devfuse_partial (allocated on first use): the partial rows of blz_dot_pair_device, twice devalg_partial's size.
 *   devsmall_stack / devsmall_ctl (allocated on first use): the partial echelons and control words of blz_rref_device, never
 *   the rref_* buffers of blz_block_rref / blz_kernel_basis.
 */
#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>

#include "blz_internal.h"
#include "blz_kernels.h"
#include "blz_border.h"
#include "blz_devio.h"
#include "blz_devalg.h"
#include "blz_devsmall.h"
#include "blz_devrank.h"
#include "blz_devw32.h"
#include "blz_devmfma.h"
#include "blz_devmat.h"
#include "blz_devorder.h"
#include "blz_devrhs.h"

#define HIPCHK(expr)                                                                                     \
	do {                                                                                             \
		hipError_t e_ = (expr);                                                                  \
		if (e_ != hipSuccess)                                                                    \
			return blz_fail(BLZ_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
	} while (0)

namespace {

struct Rccl {
	void *handle = nullptr;
	ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
	ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
	ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
	ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
	ncclResult_t (*ReduceScatter)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
	const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;

/* RCCL is resolved at run time and only when a communicator is asked for: a single-GPU solve has
 * no dependency on it. */
int rccl_load()
{
	/* the CLI's --gpus N has one thread per GPU, each asking for its communicator: one of them loads, the others wait */
	static std::mutex load_mu;
	std::lock_guard<std::mutex> lk(load_mu);
	if (g_rccl.handle)
		return BLZ_OK;
	/* Prefer the RCCL that belongs to the ROCm installation this library was built against (the HIP runtime the
	 * process uses is /opt/rocm's when libblz_hip.so is loaded first); BLZ_RCCL_PATH overrides; a copy already
	 * mapped under the plain soname (e.g. torch's) is the last resort. */
	const char *names[] = { getenv("BLZ_RCCL_PATH"), "/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so" };
	void *h = nullptr;
	for (const char *nm : names)
		if (nm && nm[0] && (h = dlopen(nm, RTLD_NOW | RTLD_LOCAL)))
			break;
	if (!h)
		return blz_fail(BLZ_ECOMM, "cannot load librccl: %s", dlerror());
#define SYM(field, name)                                                                   \
	*(void **)(&g_rccl.field) = dlsym(h, name);                                        \
	if (!g_rccl.field)                                                                 \
		return blz_fail(BLZ_ECOMM, "librccl lacks %s", name);
	SYM(GetUniqueId, "ncclGetUniqueId")
	SYM(CommInitRank, "ncclCommInitRank")
	SYM(CommDestroy, "ncclCommDestroy")
	SYM(AllGather, "ncclAllGather")
	SYM(AllReduce, "ncclAllReduce")
	SYM(ReduceScatter, "ncclReduceScatter")
	SYM(CommCount, "ncclCommCount")
	SYM(CommUserRank, "ncclCommUserRank")
	SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
	g_rccl.handle = h;
	return BLZ_OK;
}

#define NCCLCHK(expr)                                                                                     \
	do {                                                                                              \
		ncclResult_t r_ = (expr);                                                                 \
		if (r_ != ncclSuccess)                                                                    \
			return blz_fail(BLZ_ECOMM, "%s: %s", #expr, g_rccl.GetErrorString(r_));           \
	} while (0)

}  // namespace

enum { PK_SPMV1 = 0, PK_SPMV2, PK_DOT, PK_SEMI, PK_ORTHO, PK_AG_V, PK_AG_T, PK_AR, PK_RS, PK_COUNT };

/*
 * Loopback communicator (round 3): several contexts of ONE process on ONE device, one host thread each, exchange through
 * this object instead of RCCL (which refuses two ranks on one GPU).  Everything else of the multi-rank path -- the slabs,
 * the gathered layouts, the piece pipeline on two streams with its events, the landing buffers, what a batch does past
 * the stop -- is the production code, so the one-GPU boxes this was developed on can run blz_iterate with 2, 3 or 8 real
 * ranks' worth of sums against the oracle.  A collective is: post my buffers and an event on my stream; meet the other
 * threads; make my stream wait for their events and enqueue my copies / sums from THEIR send buffers; record a second
 * event; meet again; make my stream wait for everybody's second event (nobody overwrites a buffer somebody still reads).
 * Not a transport: the data never leaves the device.
 */
struct blz_loop_group {
	int nranks = 0;
	std::mutex mu;
	std::condition_variable cv;
	int arrived = 0;
	unsigned long long generation = 0;
	bool broken = false;
	int timeout_s = 120;		/* BLZ_LOOP_TIMEOUT_S at creation (tests of the time-out itself) */
	std::vector<const void *> send;
	/* one pair of events per rank, OWNED BY THE GROUP and destroyed with it: a rank that is done may destroy its context
	 * while a peer's stream still holds a wait on its event that has not executed yet */
	std::vector<hipEvent_t> ready, done;
	/* all ranks meet; false after the time-out or once any rank has given up */
	bool meet()
	{
		std::unique_lock<std::mutex> lk(mu);
		if (broken)
			return false;
		const unsigned long long gen = generation;
		if (++arrived == nranks) {
			arrived = 0;
			generation++;
			cv.notify_all();
			return true;
		}
		if (!cv.wait_for(lk, std::chrono::seconds(timeout_s), [&] { return generation != gen || broken; }))
			broken = true;
		if (broken) {
			cv.notify_all();
			return false;
		}
		return true;
	}
};

struct ProfSpan {
	int cls;
	hipEvent_t a, b;
};

/*
 * The border of a solve with right-hand sides: the matrix has k extra empty rows / columns, the last
 * k of side 0 in the original numbering, and the k columns of b are applied behind each product (enqueue_border).  Every
 * entry point leaves it through border_install, and while a border is resident (rhs != nullptr), for every k:
 *   k >= 1, and row_words = the words per row of rhs: 1 for k = 1, border_kp(k) (zero padded) otherwise;
 *   rhs = one row of row_words words of the context's width per row of side 1 that this rank holds, solver's numbering;
 *   rows[i], rows_dev[i], i < k = border row i's position in the operand a product of side 0 reads: its row in the solver's
 *     numbering on one rank, its position in the GATHERED operand on several (blz_gathered_position);
 *   distributed = set by blz_set_rhs_ranks on a context with a communicator; then own[i], own_dev[i], i < k = the local row
 *     of border row i where this rank owns it, -1 elsewhere, send = the rank's k x n share of the border dot and recv = where
 *     its all-reduce lands (k_border_place reads it while the stop flag is down: allreduce_dots' rule);
 *   partial_words = the room in `partial`, at least border_dot_max_blocks * row_words * BLZ_BORDER_MAXN.
 * rows_dev and own_dev hold BLZ_MAX_RHS entries, send and recv BLZ_MAX_RHS x cfg.n words; they and `partial` outlive the
 * border (border_release keeps them until the context goes).
 */
struct Border {
	void *rhs = nullptr;
	int k = 0, row_words = 0;
	std::vector<int64_t> rows, own;
	long long *rows_dev = nullptr, *own_dev = nullptr;
	bool distributed = false;
	u64 *partial = nullptr;		/* partial rows of the border dot */
	size_t partial_words = 0;
	u64 *send = nullptr, *recv = nullptr;
};

struct blz_ctx {
	bool profiling = false;
	std::vector<ProfSpan> spans;
	std::vector<hipEvent_t> pool;
	int device = 0;
	KernelCfg cfg{};
	u64 prime = 0;
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	bool have_matrix = false;
	bool values_wide = false;	/* wide value mode: the matrix was (or the next one will be) set with high limbs; one rank, one piece */
	const u32 *wide_hi = nullptr;	/* borrowed until the next matrix-setting call has consumed it */
	int64_t wide_nnz = 0;
	bool values_signed = false;	/* signed value mode: matrix values are int32 bit patterns, an entry a means a mod p */
	int right = 0, rank = 0, nranks = 1;
	int64_t glob_rows[2] = { 0, 0 };		/* side 0: N, side 1: C */
	int64_t first[2] = { 0, 0 }, count[2] = { 0, 0 }, stride[2] = { 0, 0 };
	std::vector<int64_t> bounds[2];
	std::vector<DevCsr> csr[2];			/* column pieces of this rank's rows of M / M^T */
	int row_side[2] = { 0, 1 };			/* side of the rows of csr[t] */
	/* slab[APPLY_SLAB + side] (hidden block numbers, never a caller's): the two scratch slabs of blz_apply_device */
	void *slab[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
	size_t slab_bytes[6] = { 0, 0, 0, 0, 0, 0 };	/* several ranks: each block sized by its own side (V, AV, P: rows of v; TMP: the other side) */
	void *gath[2] = { nullptr, nullptr };		/* gathered operands (nranks > 1) */
	int gath_holds[2] = { -1, -1 };			/* which block each one currently holds */
	int ag_chunks = 0;				/* pieces per all-gather: BLZ_AG_CHUNKS, 0 = choose from the slab size */
	hipStream_t xstream = nullptr;			/* exchange stream (all-gathers run beside the products) */
	hipEvent_t ev_prod = nullptr;			/* the producer of the block to exchange has been enqueued */
	std::vector<hipEvent_t> ev_piece;		/* piece k of the exchange has landed */
	u64 *small = nullptr, *partial = nullptr;
	u64 *dot_send = nullptr;	/* this rank's vtAv | vtAAv before the all-reduce (several ranks): 2 n^2 words */
	u64 *dot_recv = nullptr;	/* where the all-reduce lands: sums of the ranks' residues; the semi-inverse kernel reads them
					 * and writes residues to `small` -- unless the stop flag is up (round 3) */
	int max_dot_blocks = 0;
	DevCtl *ctl = nullptr;
	DevCtl host_ctl{};
	DevCtl *ctl_pinned = nullptr, *ctl_pinned_dev = nullptr;	/* host-mapped landing place of the control words */
	ncclComm_t comm = nullptr;
	blz_loop_group *loop = nullptr;		/* loopback communicator instead of RCCL (contexts of one process on one device) */
	int loop_rank = -1;			/* this context's rank in it (the matrix must be set with the same rank and rank count) */
	/* perm[side][original row] = row in the solver's numbering (empty = identity); inv is the inverse */
	std::vector<int32_t> perm[2], inv[2];
	bool reorder = true;		/* BLZ_NO_REORDER=1 keeps the file's numbering */
	bool pack = true;		/* BLZ_NO_PACK=1 keeps col_idx and val as two arrays */
	bool fuse_dot = true;		/* BLZ_NO_FUSE=1 keeps block_dot as its own kernel (A/B measurements) */
	bool selfdot = true;		/* BLZ_NO_SELFDOT=1: the iteration never takes the self-dot path (selfdot_path; A/B measurements) */
	u64 *partial_self = nullptr;	/* partial rows of v^T Av out of the first product on that path: max_self_blocks x n^2 words */
	int max_self_blocks = 0;
	bool fuse_local_off = false;	/* this matrix: the second product runs the staged form and block_dot its own kernel (gathers that hit) */
	int un = 0;			/* the caller's block width; cfg.n is the width in HBM (below) */
	bool use_graph = false;		/* BLZ_GRAPH=1: single-GPU iterations are replayed from a captured hipGraph */
	bool explicit_p = false;	/* BLZ_EXPLICIT_P=1: the iteration writes p every step (A/B against the rotating form) */
	/* the rotating form of the iteration (enqueue_iteration) leaves p as X * E: X = slab[BLZ_P] (the v of the step before,
	 * untouched), E n x n in `small`.  Set while that may be so; materialize_p() makes slab[BLZ_P] = p again */
	bool p_implicit = false;
	long long rot_swaps = 0;	/* swaps of slab[BLZ_V] / slab[BLZ_P] by the batch being enqueued (blz_iterate) */
	hipGraphExec_t iter_graph = nullptr;
	bool external_exchange = false;
	bool force_comm = false;	/* BLZ_FORCE_COMM=1: issue the collectives even on one rank (plumbing test) */
	/* asynchronous snapshot of v and p (checkpoints): pinned staging, its own stream, one in flight */
	hipStream_t cstream = nullptr;
	hipEvent_t ev_snap_go = nullptr, ev_snap_done = nullptr;
	void *snap_host[2] = { nullptr, nullptr };
	void *snap_dev[2] = { nullptr, nullptr };	/* device-side copy the D2H reads from while the loop goes on (nullptr: no room) */
	size_t snap_bytes = 0;
	std::atomic<bool> snap_pending{ false };	/* set by the owner (begin), cleared by whoever collects (wait: possibly another thread) */
	int64_t snap_iterations = 0;
	/* short-side exchange (tall / wide matrices on several ranks): product t multiplies the transpose of this rank's rows
	 * of the other orientation by its OWN slab and reduce-scatters the full-length partial products */
	bool short_side[2] = { false, false };
	DevCsr csr_short[2];
	void *part = nullptr;		/* partial product, nranks x stride[output side] rows (u64 words) */
	size_t part_bytes = 0;
	void *rs_recv = nullptr;	/* where the reduce-scatter of `part` lands (stride rows); k_reduce_modp copies it into the slab
					 * as residues unless the stop flag is up (round 3) */
	size_t rs_bytes = 0;
	double hot_share[2] = { 0.0, 0.0 };	/* share of the entries held by the rows / columns numbered first */
	double locality[2] = { 1.0, 1.0 };	/* lines per gathered entry in windows of rows, product M*x / M^T*x */
	int order_kind = 0;			/* which order blz_reorder_auto chose */
	/* blz_block_rref / blz_kernel_basis (allocated on first use) */
	u64 *rref_stack = nullptr;	/* partial echelons: num_cu * 2 workgroups x n rows x n words */
	u64 *rref_gath = nullptr;	/* every rank's echelon (nranks x n x n) */
	u64 *rref_out = nullptr;	/* the RREF, n x n */
	u64 *rref_z = nullptr;		/* n x n operand of the block product */
	int *rref_ctl = nullptr;	/* [rank-n flag, stacked rows, rank, pivots[n]] */
	Border bd;			/* the border of a solve with right-hand sides (above) */
	/* device blocks (blz_set_block_device, blz_get_block_device, blz_apply_device) */
	int32_t *inv_dev[2] = { nullptr, nullptr };	/* inv[side] on the device: uploaded on first use, freed with the matrix */
	bool inv_ready = false;
	hipEvent_t ev_caller = nullptr, ev_ours = nullptr;	/* the caller's stream has reached the call / our work is enqueued */
	unsigned long long *bad_dev = nullptr;		/* words not below p seen by a validating import */
	DevCtl *apply_ctl = nullptr;			/* control words of blz_apply_device's products: the stop flag never up */
	/* device block algebra (blz_dot_device): dev_dot_max_blocks() partial rows of un * un words, allocated on first use */
	u64 *devalg_partial = nullptr;
	/* fused device calls (blz_dot_pair_device): dev_dot_max_blocks() partial rows of 2 * un * un words, allocated on first use */
	u64 *devfuse_partial = nullptr;
	/* device block algebra on the matrix cores (blz_devmfma.hip): the rows from which each (call, width) takes that form
	 * (BLZ_DEV_MFMA_MIN_ROWS, or the measured defaults), and the digit image of a recombination's coefficients,
	 * dm_image_bytes_max() = 132 096 bytes, allocated on first use.  The inner products use the partial rows above. */
	int64_t devmfma_min_rows[DM_NOPS][2] = {};
	unsigned char *devmfma_img = nullptr;
	/* device small algebra (blz_rref_device): dev_rref_stack_rows() partial echelon rows of un words and [rank-n flag, rows
	 * stacked], allocated on first use */
	u64 *devsmall_stack = nullptr;
	int *devsmall_ctl = nullptr;
	/* device blocks on ranks (blz_set_device_ranks): the blocks of the device-block family are this
	 * rank's own rows in slab order.  devrank_send = the rank's residues of a dot (2 un * un words), devrank_recv = where
	 * their all-reduce lands; both this family's own (never dot_send / dot_recv), allocated on first use */
	bool device_ranks = false;
	u64 *devrank_send = nullptr, *devrank_recv = nullptr;
	/* the resident matrix was built on the device (blz_set_matrix_device / blz_set_matrix_upload) */
	bool device_built = false;
	/* ... and renumbered there first (blz_set_matrix_device_ordered with order 1) */
	bool device_order = false;
};

enum { APPLY_SLAB = 4 };
static void devio_release_matrix(blz_ctx *c);

/* no border is resident from here on; scratch_too: the context goes, and the tables and buffers that outlive a border with it */
static void border_release(blz_ctx *c, bool scratch_too)
{
	Border &B = c->bd;
	if (B.rhs)
		hipFree(B.rhs);
	B.rhs = nullptr;
	B.k = B.row_words = 0;
	B.rows.clear();
	B.own.clear();
	B.distributed = false;
	if (!scratch_too)
		return;
	for (void *q : { (void *)B.partial, (void *)B.rows_dev, (void *)B.own_dev, (void *)B.send, (void *)B.recv })
		if (q)
			hipFree(q);
	B.partial = B.send = B.recv = nullptr;
	B.rows_dev = B.own_dev = nullptr;
	B.partial_words = 0;
}

/* HIP-event span around one enqueue on the context's stream (only while profiling is on). */
struct Span {
	blz_ctx *c;
	hipEvent_t b = nullptr;
	hipStream_t st;
	Span(blz_ctx *ctx, int cls, hipStream_t on = nullptr) : c(ctx), st(on ? on : ctx->stream)
	{
		if (!c->profiling)
			return;
		hipEvent_t ev[2];
		for (auto &e : ev) {
			if (!c->pool.empty()) {
				e = c->pool.back();
				c->pool.pop_back();
			} else if (hipEventCreate(&e) != hipSuccess) {
				return;
			}
		}
		(void)hipEventRecord(ev[0], st);
		b = ev[1];
		c->spans.push_back(ProfSpan{ cls, ev[0], ev[1] });
	}
	~Span()
	{
		if (b)
			(void)hipEventRecord(b, st);
	}
};

/* (the scratch slab of side 1 counts: on ranks enqueue_product gathers by the side of its source) */
static inline int side_of(int block) { return block == BLZ_TMP || block == APPLY_SLAB + 1 ? 1 : 0; }

static inline char *slab_ptr(const blz_ctx *c, int block) { return (char *)c->slab[block]; }

/* the operand a product reads when its source is `block`: the slab itself on one rank, else the gathered copy */
static inline const void *operand_ptr(const blz_ctx *c, int block)
{
	return c->nranks == 1 ? c->slab[block] : c->gath[side_of(block)];
}

/* p is slab[BLZ_P] as it stands: E <- I, flags down.  (Synchronous: outside the loop only.) */
static int explicit_p_state(blz_ctx *c)
{
	const int np = c->cfg.n;
	std::vector<u64> tail((size_t)(small_words(np) - small_E(np)), 0);
	for (int i = 0; i < np; i++)
		tail[(size_t)i * np + i] = 1;
	HIPCHK(hipStreamSynchronize(c->stream));
	HIPCHK(hipMemcpy(c->small + small_E(np), tail.data(), tail.size() * sizeof(u64), hipMemcpyHostToDevice));
	c->p_implicit = false;
	return BLZ_OK;
}

/* slab[BLZ_P] <- X * E = p and E <- I, before anything outside the loop looks at p.  E is read from device memory (the
 * host never learns it) and the pass does not look at the stop flag: p is the same block before and after the stop. */
static int materialize_p(blz_ctx *c)
{
	if (!c->p_implicit)
		return BLZ_OK;
	const int np = c->cfg.n;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(launch_block_mul(c->cfg, c->slab[BLZ_P], c->count[0], np, np, c->small + small_E(np), c->stream));
	return explicit_p_state(c);
}

static void free_csr(DevCsr &A)
{
	if (A.row_ptr) hipFree(A.row_ptr);
	if (A.col_idx) hipFree(A.col_idx);
	if (A.val) hipFree(A.val);
	if (A.val_hi) hipFree(A.val_hi);
	if (A.palette) hipFree(A.palette);
	if (A.heavy) hipFree(A.heavy);
	if (A.heavy_multi) hipFree(A.heavy_multi);
	if (A.heavy_scratch) hipFree(A.heavy_scratch);
	if (A.medium_rows) hipFree(A.medium_rows);
	A = DevCsr{};
}

extern "C" int blz_device_count(void)
{
	int cnt = 0;
	if (hipGetDeviceCount(&cnt) != hipSuccess)
		return 0;
	return cnt;
}

extern "C" int blz_create(blz_ctx **out, int device, uint64_t prime, int n)
{
	if (!out)
		return blz_fail(BLZ_EINVAL, "blz_create: out is NULL");
	*out = nullptr;
	if (n < 1 || n > BLZ_MAX_N)
		return blz_fail(BLZ_EINVAL, "n = %d is outside 1..%d", n, BLZ_MAX_N);
	if (prime < 2 || prime >= (1ull << 62))
		return blz_fail(BLZ_EINVAL, "p must satisfy 2 <= p < 2**62 (the reference's cap of 2**30 - 35 is lifted, "
				"sequential/lanczos_modp.c:189)");
	int cnt = 0;
	if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
		return blz_fail(BLZ_ENOGPU, "no HIP device visible: libblz_hip has no CPU path");
	if (device < 0 || device >= cnt)
		return blz_fail(BLZ_EINVAL, "device %d out of range (%d visible)", device, cnt);
	HIPCHK(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, device));
	blz_ctx *c = new blz_ctx();
	c->device = device;
	c->prime = prime;
	/* Blocks live in HBM with the width rounded up to a power of two, the extra columns zero: block rows are then
	 * aligned to the 128-byte lines the gathers fetch, and every width runs the specialised kernels of the next
	 * power of two.  Zero columns stay zero through every step (they are never pivots, their coefficients are zero),
	 * so the caller's n columns are the reference's.  BLZ_NO_PAD=1 keeps the exact width (generic kernels). */
	c->un = n;
	c->cfg.n = n;
	{
		const char *npad = getenv("BLZ_NO_PAD");
		if (!(npad && npad[0] == '1'))
			while (c->cfg.n & (c->cfg.n - 1))
				c->cfg.n++;
	}
	const int np_ = c->cfg.n;
	c->cfg.word = prime < (1ull << 32) ? 4 : 8;
	c->cfg.mers = modp_mersenne(prime);
	c->cfg.m = make_modp(prime);
	c->cfg.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	c->cfg.spmv_blocks_per_cu = 0;	/* 0 = choose from the row length */
	if (const char *bp = getenv("BLZ_SPMV_BLOCKS_PER_CU"))
		if (atoi(bp) >= 1 && atoi(bp) <= 64)
			c->cfg.spmv_blocks_per_cu = atoi(bp);
	{
		const char *ns = getenv("BLZ_NO_STAGE");
		c->cfg.staged = !(ns && ns[0] == '1');
		const char *su = getenv("BLZ_STAGE_U");		/* gathers in flight per lane of the staged SpMV: 4 / 8 (A/B); 0 = by plan */
		c->cfg.stage_u = su ? atoi(su) : 0;
		const char *npr = getenv("BLZ_NO_PAIR");
		c->cfg.pair = !(npr && npr[0] == '1');
		const char *sdy = getenv("BLZ_STAGE_DYN");
		c->cfg.stage_dyn = sdy ? (sdy[0] == '1' ? 1 : 0) : -1;
	}
	{
		const char *nsd = getenv("BLZ_NO_SIDE");
		c->cfg.side = nullptr;
		c->cfg.ev_fork = c->cfg.ev_join = nullptr;
		if (!(nsd && nsd[0] == '1')) {
			HIPCHK(hipStreamCreateWithFlags(&c->cfg.side, hipStreamNonBlocking));
			HIPCHK(hipEventCreateWithFlags(&c->cfg.ev_fork, hipEventDisableTiming));
			HIPCHK(hipEventCreateWithFlags(&c->cfg.ev_join, hipEventDisableTiming));
		}
	}
	{
		const char *nm = getenv("BLZ_NO_MFMA");
		c->cfg.mfma = !(nm && nm[0] == '1');
		/* measured on MI355X: fixed cost 18 us vs 9 us, slope 52 vs 71 us per million rows at n = 8 (cross at 0.5 M rows);
		 * at n = 16 the vector kernel is compute-bound at 255 us per million rows (cross near 0.1 M rows) */
		const char *s8 = getenv("BLZ_MFMA_STAGE8");
		c->cfg.mfma_stage8 = s8 && s8[0] == '1';
		const char *mr = getenv("BLZ_MFMA_MIN_ROWS");
		c->cfg.mfma_min_rows = mr ? atoll(mr) : (n == 16 ? 100000 : 500000);
		/* the device block algebra's own switch: one row count for every call kind and width, 0 = always */
		const char *dmr = getenv("BLZ_DEV_MFMA_MIN_ROWS");
		for (int op = 0; op < DM_NOPS; op++)
			for (int w = 0; w < 2; w++)
				c->devmfma_min_rows[op][w] = dmr ? (int64_t)atoll(dmr) : dm_default_min_rows(op, w ? 16 : 8);
		c->cfg.mfma_img = nullptr;
		HIPCHK(hipMalloc(&c->cfg.mfma_img, ortho_mfma_image_bytes()));
	}
	{
		const char *npn = getenv("BLZ_NO_PANEL");
		c->cfg.panel = !(npn && npn[0] == '1');
	}
	const char *np = getenv("BLZ_NO_PACK");
	c->pack = !(np && np[0] == '1');
	const char *nr = getenv("BLZ_NO_REORDER");
	c->reorder = !(nr && nr[0] == '1');
	const char *nf = getenv("BLZ_NO_FUSE");
	c->fuse_dot = !(nf && nf[0] == '1');
	const char *nsf = getenv("BLZ_NO_SELFDOT");
	c->selfdot = !(nsf && nsf[0] == '1');
	const char *ug = getenv("BLZ_GRAPH");
	c->use_graph = ug && ug[0] == '1';
	const char *xp = getenv("BLZ_EXPLICIT_P");
	c->explicit_p = xp && xp[0] == '1';
	if (const char *ac = getenv("BLZ_AG_CHUNKS"))
		if (atoi(ac) >= 1 && atoi(ac) <= 64)
			c->ag_chunks = atoi(ac);
	HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
	HIPCHK(hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking));
	HIPCHK(hipEventCreateWithFlags(&c->ev_prod, hipEventDisableTiming));
	HIPCHK(hipEventCreate(&c->ev0));
	HIPCHK(hipEventCreate(&c->ev1));
	HIPCHK(hipMalloc(&c->small, small_words(np_) * sizeof(u64)));
	HIPCHK(hipMemset(c->small, 0, small_words(np_) * sizeof(u64)));
	{
		int rc_ = explicit_p_state(c);
		if (rc_ != BLZ_OK)
			return rc_;
	}
	HIPCHK(hipMalloc(&c->dot_send, (size_t)2 * np_ * np_ * sizeof(u64)));
	HIPCHK(hipMemset(c->dot_send, 0, (size_t)2 * np_ * np_ * sizeof(u64)));
	HIPCHK(hipMalloc(&c->dot_recv, (size_t)2 * np_ * np_ * sizeof(u64)));
	HIPCHK(hipMemset(c->dot_recv, 0, (size_t)2 * np_ * np_ * sizeof(u64)));
	/* partial rows of the inner products: the fused path (n <= 8) needs room for the streaming kernel plus the
	 * outlier launches; the stand-alone kernel keeps the grid it was tuned with */
	c->max_dot_blocks = c->cfg.num_cu * (np_ <= 8 ? 16 : 8);
	HIPCHK(hipMalloc(&c->partial, (size_t)c->max_dot_blocks * 2 * np_ * np_ * sizeof(u64)));
	if (c->selfdot && np_ <= 8) {	/* one row per workgroup of the first product: at most 8 per CU unless the experiment knob asks for more */
		c->max_self_blocks = c->cfg.num_cu * std::max(8, c->cfg.spmv_blocks_per_cu) + 8;
		HIPCHK(hipMalloc(&c->partial_self, (size_t)c->max_self_blocks * np_ * np_ * sizeof(u64)));
	}
	HIPCHK(hipMalloc(&c->ctl, sizeof(DevCtl)));
	HIPCHK(hipHostMalloc((void **)&c->ctl_pinned, sizeof(DevCtl), hipHostMallocMapped));
	HIPCHK(hipHostGetDevicePointer((void **)&c->ctl_pinned_dev, c->ctl_pinned, 0));
	HIPCHK(hipMemset(c->ctl, 0, sizeof(DevCtl)));
	*out = c;
	return BLZ_OK;
}

extern "C" void blz_destroy(blz_ctx *c)
{
	if (!c)
		return;
	hipSetDevice(c->device);
	if (c->stream)
		hipStreamSynchronize(c->stream);
	if (c->xstream)
		hipStreamSynchronize(c->xstream);
	for (auto &sp : c->spans) {
		hipEventDestroy(sp.a);
		hipEventDestroy(sp.b);
	}
	for (auto &e : c->pool)
		hipEventDestroy(e);
	if (c->iter_graph)
		hipGraphExecDestroy(c->iter_graph);
	if (c->comm && g_rccl.CommDestroy)
		g_rccl.CommDestroy(c->comm);
	for (int t = 0; t < 2; t++)
		for (auto &A : c->csr[t])
			free_csr(A);
	for (auto &A : c->csr_short)
		free_csr(A);
	if (c->part) hipFree(c->part);
	devio_release_matrix(c);
	if (c->ev_caller) hipEventDestroy(c->ev_caller);
	if (c->ev_ours) hipEventDestroy(c->ev_ours);
	if (c->bad_dev) hipFree(c->bad_dev);
	if (c->devalg_partial) hipFree(c->devalg_partial);
	if (c->devfuse_partial) hipFree(c->devfuse_partial);
	if (c->devmfma_img) hipFree(c->devmfma_img);
	if (c->devsmall_stack) hipFree(c->devsmall_stack);
	if (c->devsmall_ctl) hipFree(c->devsmall_ctl);
	if (c->devrank_send) hipFree(c->devrank_send);
	if (c->devrank_recv) hipFree(c->devrank_recv);
	for (void *&b : c->slab)
		if (b) hipFree(b);
	for (void *&b : c->gath)
		if (b) hipFree(b);
	for (auto &e : c->ev_piece)
		hipEventDestroy(e);
	if (c->ev_prod) hipEventDestroy(c->ev_prod);
	if (c->xstream) hipStreamDestroy(c->xstream);
	if (c->cstream) {
		hipStreamSynchronize(c->cstream);
		hipStreamDestroy(c->cstream);
	}
	if (c->ev_snap_go) hipEventDestroy(c->ev_snap_go);
	if (c->ev_snap_done) hipEventDestroy(c->ev_snap_done);
	for (void *&h : c->snap_host)
		if (h) hipHostFree(h);
	for (void *&d : c->snap_dev)
		if (d) hipFree(d);
	if (c->small) hipFree(c->small);
	for (u64 *b : { c->rref_stack, c->rref_gath, c->rref_out, c->rref_z })
		if (b) hipFree(b);
	if (c->rref_ctl) hipFree(c->rref_ctl);
	border_release(c, true);
	if (c->dot_send) hipFree(c->dot_send);
	if (c->dot_recv) hipFree(c->dot_recv);
	if (c->rs_recv) hipFree(c->rs_recv);
	if (c->cfg.mfma_img) hipFree(c->cfg.mfma_img);
	if (c->cfg.side) {
		hipStreamSynchronize(c->cfg.side);
		hipStreamDestroy(c->cfg.side);
	}
	if (c->cfg.ev_fork) hipEventDestroy(c->cfg.ev_fork);
	if (c->cfg.ev_join) hipEventDestroy(c->cfg.ev_join);
	if (c->partial) hipFree(c->partial);
	if (c->partial_self) hipFree(c->partial_self);
	if (c->ctl) hipFree(c->ctl);
	if (c->ctl_pinned) hipHostFree(c->ctl_pinned);
	if (c->ev0) hipEventDestroy(c->ev0);
	if (c->ev1) hipEventDestroy(c->ev1);
	if (c->stream) hipStreamDestroy(c->stream);
	delete c;
}

extern "C" int blz_word_bytes(const blz_ctx *c) { return c ? c->cfg.word : 0; }

extern "C" int blz_set_values_signed(blz_ctx *c, int on)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_set_values_signed: NULL context");
	if (c->have_matrix)
		return blz_fail(BLZ_EINVAL, "blz_set_values_signed: a matrix is resident; choose the value mode before the matrix is set");
	if (on && c->values_wide)
		return blz_fail(BLZ_EINVAL, "blz_set_values_signed: the context is in wide value mode; the two never combine");
	c->values_signed = on != 0;
	return BLZ_OK;
}

static int wide_refuse_ranks(const blz_ctx *c, const char *who, int nranks)
{
	if (nranks > 1 || c->comm || c->loop || c->force_comm)
		return blz_fail(BLZ_EINVAL, "%s: wide matrix entries need a single rank in one piece, without a communicator, a loopback "
				"group or BLZ_FORCE_COMM (the high limbs are not distributed: see DESIGN.md section 14)", who);
	return BLZ_OK;
}

extern "C" int blz_set_values_wide(blz_ctx *c, const uint32_t *x_hi, int64_t nnz)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_set_values_wide: NULL context");
	if (c->have_matrix)
		return blz_fail(BLZ_EINVAL, "blz_set_values_wide: a matrix is resident; hand the high limbs over before the matrix is set");
	if (!x_hi) {
		c->values_wide = false;
		c->wide_hi = nullptr;
		c->wide_nnz = 0;
		return BLZ_OK;
	}
	if (c->values_signed)
		return blz_fail(BLZ_EINVAL, "blz_set_values_wide: the context is in signed value mode; the two never combine");
	if (nnz < 0)
		return blz_fail(BLZ_EINVAL, "blz_set_values_wide: nnz = %lld", (long long)nnz);
	const int rc = wide_refuse_ranks(c, "blz_set_values_wide", 1);
	if (rc != BLZ_OK)
		return rc;
	c->values_wide = true;
	c->wide_hi = x_hi;
	c->wide_nnz = nnz;
	return BLZ_OK;
}

extern "C" int blz_values_wide(const blz_ctx *c) { return c && c->values_wide ? 1 : 0; }

extern "C" int blz_values_signed(const blz_ctx *c) { return c && c->values_signed ? 1 : 0; }

static int plan_csr(blz_ctx *c, const u32 *row_ptr, DevCsr &D, int64_t hot_rows, bool dot_slab);

/* product t's (last) launch carries the inner products where that form exists: product `right` is the second one of the iteration */
static inline bool carries_dots(const blz_ctx *c, int t) { return t == c->right && c->fuse_dot && spmv_dot_supported(c->cfg); }

/* a wide slab sums a row's products unreduced (csrc/modp.h): what both paths refuse before they build one */
static int wide_refuse_long_row(const u32 *row_ptr, int64_t rows)
{
	for (int64_t r = 0; r < rows; r++)
		if (row_ptr[r + 1] - row_ptr[r] > (1u << 30))
			return blz_fail(BLZ_EINVAL, "a row of a wide slab has more than 2^30 entries: its unreduced sum is not bounded "
					"(csrc/modp.h)");
	return BLZ_OK;
}

/* The stream arrays of a slab of nnz entries: col_idx always, val and val_hi on request.  The streaming kernels read up to
 * BLZ_STREAM_PAD elements past the end of each, so each has nnz + BLZ_STREAM_PAD elements and its pad is zeroed, on `st`.
 * Every matrix-setting call ends in matrix_blocks, which synchronises c->stream: named here, the pad is zero before the call
 * returns to its caller. */
static int alloc_stream_arrays(DevCsr &D, int64_t nnz, bool val, bool val_hi, hipStream_t st)
{
	void **const arr[3] = { (void **)&D.col_idx, val ? (void **)&D.val : nullptr, val_hi ? (void **)&D.val_hi : nullptr };
	for (void **a : arr) {
		if (!a)
			continue;
		HIPCHK(hipMalloc(a, (size_t)(nnz + BLZ_STREAM_PAD) * sizeof(u32)));
		HIPCHK(hipMemsetAsync((u32 *)*a + nnz, 0, BLZ_STREAM_PAD * sizeof(u32), st));
	}
	return BLZ_OK;
}

/* hi0: wide value mode, the high limbs of H0.val (host) */
static int upload_csr(blz_ctx *c, const blz_csr &H0, DevCsr &D, int64_t hot_rows = 0, bool dot_slab = false, double locality = 1.0,
		      const u32 *hi0 = nullptr)
{
	free_csr(D);
	/* Signed value mode: H0.val holds int32 bit patterns.  64-bit words: they travel as they are and the slab's products run
	 * the signed instantiations -- unless no entry is negative, when the pattern IS the residue and the unsigned ones do.
	 * 4-byte words (p < 2^32): a mod p fits a u32, so the values are canonicalised here and today's kernels run. */
	blz_csr H = H0;
	std::vector<u32> canon;
	bool sgn = false;
	if (c->values_signed && H0.val) {
		if (c->cfg.word == 8) {
			for (int64_t k = 0; k < H0.nnz && !sgn; k++)
				sgn = (int32_t)H0.val[k] < 0;
		} else {
			canon.resize((size_t)H0.nnz);
			const int64_t p = (int64_t)c->prime;
			for (int64_t k = 0; k < H0.nnz; k++) {
				const int64_t r = (int64_t)(int32_t)H0.val[k] % p;
				canon[(size_t)k] = (u32)(r < 0 ? r + p : r);
			}
			H.val = canon.data();
		}
	}
	D.sgn = sgn;
	/* Wide value mode: the slab runs the wide instantiations only when it really has an entry with a non-zero high limb (and
	 * the words are 8 bytes: below 2^32 no residue has one).  Otherwise the high array is dropped and today's kernels run. */
	const u32 *hi = nullptr;
	if (hi0 && H0.val && c->cfg.word == 8) {
		for (int64_t k = 0; k < H0.nnz && !hi; k++)
			if (hi0[k])
				hi = hi0;
	}
	if (hi) {
		const int rcw = wide_refuse_long_row(H0.row_ptr, H0.rows);
		if (rcw != BLZ_OK)
			return rcw;
	}
	D.wide = hi != nullptr;
	D.locality = locality;
	D.rows = H.rows;
	D.cols = H.cols;
	D.nnz = H.nnz;
	HIPCHK(hipMalloc(&D.row_ptr, (size_t)(H.rows + 1) * sizeof(u32)));
	HIPCHK(hipMemcpy(D.row_ptr, H.row_ptr, (size_t)(H.rows + 1) * sizeof(u32), hipMemcpyHostToDevice));
	/* Packed stream: when the slab has at most 256 distinct values and fewer than 2^24 columns, each entry
	 * travels as ONE u32 (column | palette index << 24) instead of two; the SpMV is bound by the number of
	 * fabric requests, and this halves those of the matrix stream.  BLZ_NO_PACK=1 keeps the plain arrays. */
	bool packed = false;
	std::vector<u32> pal, pk;
	if (H.val && c->pack && H.cols < (1 << 24)) {
		std::vector<u32> pal_hi;	/* (wide: 256 low limbs, then 256 high limbs) */
		pk.resize((size_t)H.nnz);
		std::vector<int> slot(4096, -1);	/* open-addressing hash: value -> palette index */
		packed = true;
		for (int64_t k = 0; k < H.nnz && packed; k++) {
			const u32 v = H.val[k], vh = hi ? hi[k] : 0u;
			u32 h = ((v ^ vh * 0x9E3779B1u) * 2654435761u) >> 20;
			while (slot[h] >= 0 && (pal[(size_t)slot[h]] != v || (hi && pal_hi[(size_t)slot[h]] != vh)))
				h = (h + 1) & 4095u;
			if (slot[h] < 0) {
				if (pal.size() == 256) {
					packed = false;
					break;
				}
				slot[h] = (int)pal.size();
				pal.push_back(v);
				if (hi)
					pal_hi.push_back(vh);
			}
			pk[(size_t)k] = (u32)H.col_idx[k] | ((u32)slot[h] << 24);
		}
		if (packed) {
			pal.resize(256, 0);
			if (hi) {
				pal_hi.resize(256, 0);
				pal.insert(pal.end(), pal_hi.begin(), pal_hi.end());
			}
		}
	}
	/* (a packed slab has no value array: its values are in the palette) */
	const int rca = alloc_stream_arrays(D, H.nnz, !packed && H.val, !packed && hi, c->stream);
	if (rca != BLZ_OK)
		return rca;
	if (packed) {
		HIPCHK(hipMalloc(&D.palette, pal.size() * sizeof(u32)));
		HIPCHK(hipMemcpy(D.palette, pal.data(), pal.size() * sizeof(u32), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(D.col_idx, pk.data(), (size_t)H.nnz * sizeof(u32), hipMemcpyHostToDevice));
	} else {
		HIPCHK(hipMemcpy(D.col_idx, H.col_idx, (size_t)H.nnz * sizeof(int), hipMemcpyHostToDevice));
		if (H.val)
			HIPCHK(hipMemcpy(D.val, H.val, (size_t)H.nnz * sizeof(u32), hipMemcpyHostToDevice));
		if (hi)
			HIPCHK(hipMemcpy(D.val_hi, hi, (size_t)H.nnz * sizeof(u32), hipMemcpyHostToDevice));
	}
	return plan_csr(c, H.row_ptr, D, hot_rows, dot_slab);
}

/* The plan of a slab whose arrays are in place (rows, cols, nnz, val, palette, wide, locality set), from a host copy of its
 * row pointers: the outlier lists, the spread of the rows the streaming kernel keeps, the staged and the panel plan.  Shared
 * by the host upload above and the device build (devmat_build). */
static int plan_csr(blz_ctx *c, const u32 *row_ptr, DevCsr &D, int64_t hot_rows, bool dot_slab)
{
	struct { int64_t rows, nnz; const u32 *row_ptr; } H = { D.rows, D.nnz, row_ptr };
	D.heavy_thr = spmv_heavy_threshold(c->cfg, H.rows, H.nnz);
	std::vector<HeavySeg> heavy;
	std::vector<HeavyRow> multi;
	std::vector<int> medium;
	int G = 1;
	while (G < c->cfg.n)
		G <<= 1;
	/* up to 256 entries per lane group of the wavefront (64 batches of 4 gathers); with one group per wavefront
	 * (n > 32) the tier is empty */
	const u32 medium_max = G < 64 ? (u32)(64 / G) * 256u : 0u;
	int64_t kept_rows = 0, kept_nnz = 0;
	double sq = 0.0;
	for (int64_t r = 0; r < H.rows; r++) {
		const u32 k0 = H.row_ptr[r], len = H.row_ptr[r + 1] - k0;
		if (len <= D.heavy_thr) {
			sq += (double)len * (double)len;
			kept_rows++;
			kept_nnz += len;
			continue;
		}
		if (len <= medium_max) {	/* one wavefront per row */
			medium.push_back((int)r);
			continue;
		}
		const u32 cnt = (len + HEAVY_SEG - 1) / HEAVY_SEG, per = (len + cnt - 1) / cnt;
		if (cnt > 1)
			multi.push_back(HeavyRow{(int)r, (int)heavy.size(), (int)cnt});
		for (u32 q = 0; q < cnt; q++)
			heavy.push_back(HeavySeg{(int)r, k0 + q * per, k0 + std::min(len, (q + 1) * per), cnt == 1});
	}
	if (kept_rows > 0) {	/* spread of the rows the streaming kernel keeps */
		const double mean = (double)kept_nnz / (double)kept_rows, var = sq / (double)kept_rows - mean * mean;
		D.uneven = var > 0.25 * mean * mean;
		D.kept_mean = mean;
	}
	D.outlier_share = H.nnz > 0 ? 1.0 - (double)kept_nnz / (double)H.nnz : 0.0;
	D.tail_batch = D.locality < 0.6 || H.nnz < 4000000;
	D.n_heavy = (int)heavy.size();
	D.n_multi = (int)multi.size();
	if (D.n_heavy) {
		HIPCHK(hipMalloc(&D.heavy, heavy.size() * sizeof(HeavySeg)));
		HIPCHK(hipMemcpy(D.heavy, heavy.data(), heavy.size() * sizeof(HeavySeg), hipMemcpyHostToDevice));
	}
	D.n_medium = (int)medium.size();
	if (D.n_medium) {
		HIPCHK(hipMalloc(&D.medium_rows, medium.size() * sizeof(int)));
		HIPCHK(hipMemcpy(D.medium_rows, medium.data(), medium.size() * sizeof(int), hipMemcpyHostToDevice));
	}
	if (D.n_multi) {
		HIPCHK(hipMalloc(&D.heavy_multi, multi.size() * sizeof(HeavyRow)));
		HIPCHK(hipMemcpy(D.heavy_multi, multi.data(), multi.size() * sizeof(HeavyRow), hipMemcpyHostToDevice));
		HIPCHK(hipMalloc(&D.heavy_scratch, heavy.size() * 64 * 2 * sizeof(u64)));
	}
	spmv_plan_staged(c->cfg, H.row_ptr, D, !dot_slab);
	spmv_plan_panel(c->cfg, H.row_ptr, D, hot_rows);
	return BLZ_OK;
}

/* the parameters a context wants its matrix prepared with (pieces per exchange, renumbering, panel capacity) */
struct PrepParams {
	int K, reorder, rows_per_line;
	int64_t hot_cap;
	double min_share;
};

static PrepParams prep_params(const blz_ctx *c, int64_t mrows, int64_t mcols, int64_t nnz, int nranks)
{
	PrepParams q;
	/* Pieces per exchange.  BLZ_AG_CHUNKS fixes it; otherwise up to 4 pieces of at least ~2 MB of the smaller
	 * block's slab (below that the collectives are latency-bound and cutting them up only adds launches).
	 * A single rank only cuts its products up when the collectives are forced on (tests). */
	q.K = 1;
	if (nranks > 1 || c->force_comm) {
		if (c->ag_chunks > 0) {
			q.K = c->ag_chunks;
		} else {
			/* Cutting a product into K pieces leaves 1/K of it exposed after the last all-gather but pays K
			 * collective start-ups (and 6-30 % more product time): exposed time
			 * T/K + K*t0 is smallest at K = sqrt(T/t0), with T = this rank's product at the measured
			 * ~55 G gathers/s and t0 ~ 25 us per all-gather call.  Pieces stay above ~2 MB per slab. */
			const int64_t rows = std::min(mrows, mcols) / nranks;
			const int64_t slab_bytes = rows * c->cfg.n * c->cfg.word;
			const double t_prod_us = (double)nnz / nranks / 55e3, t0_us = 25.0;
			const int64_t by_time = (int64_t)(std::sqrt(t_prod_us / t0_us) + 0.5);
			q.K = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(4, by_time), slab_bytes / (2 << 20)));
		}
	}
	const char *ao = getenv("BLZ_REORDER_PLAIN");	/* 1: round 1's order without the scored choice (A/B) */
	q.reorder = !c->reorder ? 0 : ((ao && ao[0] == '1') ? 2 : 1);
	q.rows_per_line = std::max(1, 128 / (c->cfg.n * c->cfg.word));
	/* densest rows / columns in front when they hold enough of the entries (one rank, products in one piece: the SpMV
	 * keeps that many block rows of its operand in LDS, k_spmv_panel) */
	q.hot_cap = 0;
	if (c->cfg.panel && nranks == 1 && q.K == 1) {
		q.hot_cap = spmv_panel_capacity(c->cfg);
		if (const char *e = getenv("BLZ_PANEL_ROWS"))
			q.hot_cap = std::min<int64_t>(q.hot_cap, std::max<int64_t>(0, atoll(e)));
	}
	q.min_share = 0.25;	/* below that the dense block rows are served from L2 at no cost to the fabric: measured on the
				 * structured workload, 17 % of the entries in the panel = no change in time */
	if (const char *e = getenv("BLZ_PANEL_MIN_PCT"))
		q.min_share = atof(e) / 100.0;
	return q;
}

extern "C" int blz_prepare_for(const blz_ctx *c, const blz_coo *M, int right, int nranks, blz_prepared **out)
{
	if (!c || !M || !out || nranks < 1)
		return blz_fail(BLZ_EINVAL, "blz_prepare_for: bad argument");
	const PrepParams q = prep_params(c, M->nrows, M->ncols, M->nnz, nranks);
	return blz_prepare(M, right, nranks, q.K, q.reorder, q.rows_per_line, q.hot_cap, q.min_share, out);
}

extern "C" uint64_t blz_prepare_key(const blz_ctx *c, uint64_t content_hash, int64_t mrows, int64_t mcols, int64_t nnz,
				    int right, int nranks)
{
	if (!c)
		return 0;
	const PrepParams q = prep_params(c, mrows, mcols, nnz, nranks);
	uint64_t h = content_hash ^ 0x9E3779B97F4A7C15ull;
	const uint64_t parts[] = { c->prime, (uint64_t)c->cfg.n, (uint64_t)c->cfg.word, (uint64_t)(right != 0), (uint64_t)nranks,
				   (uint64_t)q.K, (uint64_t)q.reorder, (uint64_t)q.rows_per_line, (uint64_t)q.hot_cap,
				   (uint64_t)(q.min_share * 1e6), (uint64_t)mrows, (uint64_t)mcols, (uint64_t)nnz, 2 /* format */ };
	for (uint64_t x : parts)
		h = (h ^ x) * 0x100000001b3ull;
	if (c->values_signed)	/* one more round in signed value mode only: the unsigned keys are what they were */
		h = (h ^ 0x5349474E45440001ull) * 0x100000001b3ull;
	return h ? h : 1;
}

/* What every matrix-setting call drops of the matrix before it: the captured iteration, the scratch of the device blocks,
 * the border.  (The first step of matrix_begin.) */
static void matrix_reset(blz_ctx *c, int right, int rank, int nranks)
{
	if (c->iter_graph) {
		hipGraphExecDestroy(c->iter_graph);
		c->iter_graph = nullptr;
	}
	devio_release_matrix(c);	/* the scratch slabs and the device copy of the numbering belong to the matrix they were made for */
	c->right = right;
	c->rank = rank;
	c->nranks = nranks;
	c->fuse_local_off = false;
	border_release(c, false);	/* a border belongs to the matrix it was set for */
}

/* what a matrix-setting call knows of its matrix before a slab of it exists */
struct MatrixShape {
	int right, rank, nranks, K;		/* K: pieces per product */
	int64_t nrows, ncols;			/* of M */
	const int64_t *bounds[2];		/* per SIDE (0: rows of v, 1: rows of tmp): nranks + 1 row bounds; NULL: one rank, the whole side */
	int64_t stride[2];			/* per side: rows of a padded slab (read with bounds only) */
	std::vector<int32_t> perm[2];		/* new index of every row / column of M; empty: the identity */
	double share[2], locality[2];		/* what the renumbering found, per product (t = 0: M * x gathers by column; t = 1: M^T * x by row) */
	int order_kind;
};

/* The first step of every matrix-setting call, the refusals behind it: the matrix that was resident goes, and the context
 * takes the geometry of the new one.  From here to the end of matrix_blocks the context has no matrix: a call that fails on
 * the way leaves it so.  csr[t] are K empty slabs, csr_short[t] is empty and no product is in its short-side form. */
static void matrix_begin(blz_ctx *c, MatrixShape &S)
{
	matrix_reset(c, S.right, S.rank, S.nranks);
	c->have_matrix = false;
	c->device_built = false;
	c->device_order = false;
	/* side 0 = rows of v: rows of M for a left kernel, columns of M for a right kernel
	 * (sequential/lanczos_modp.c:592-593). */
	const int rs = S.right ? 1 : 0, cs = 1 - rs;	/* side of M's rows / columns */
	c->glob_rows[rs] = S.nrows;
	c->glob_rows[cs] = S.ncols;
	c->row_side[0] = rs;		/* rows of M   */
	c->row_side[1] = cs;		/* rows of M^T */
	for (int sd = 0; sd < 2; sd++) {
		if (S.bounds[sd]) {
			c->bounds[sd].assign(S.bounds[sd], S.bounds[sd] + S.nranks + 1);
			c->stride[sd] = S.stride[sd];
		} else {
			c->bounds[sd].assign({ (int64_t)0, c->glob_rows[sd] });
			c->stride[sd] = c->glob_rows[sd];
		}
		c->first[sd] = c->bounds[sd][S.rank];
		c->count[sd] = c->bounds[sd][S.rank + 1] - c->bounds[sd][S.rank];
		c->perm[sd] = std::move(S.perm[sd == rs ? 0 : 1]);
		c->inv[sd].assign(c->perm[sd].size(), 0);
		for (size_t r = 0; r < c->perm[sd].size(); r++)
			c->inv[sd][(size_t)c->perm[sd][r]] = (int32_t)r;
	}
	for (int t = 0; t < 2; t++) {
		c->hot_share[t] = S.share[t];
		c->locality[t] = S.locality[t];
		for (auto &A : c->csr[t])
			free_csr(A);
		c->csr[t].assign((size_t)S.K, DevCsr{});
		free_csr(c->csr_short[t]);
		c->short_side[t] = false;
	}
	c->order_kind = S.order_kind;
}

/* The last step of every matrix-setting call, once csr[] and stride[] are what the new matrix wants: the four blocks
 * (zeroed), the gathered operands, the piece events, the control words and the explicit-p state. */
static int matrix_blocks(blz_ctx *c, int nranks, int K)
{
	/* One rank: every block can hold either side (the reference sizes all four for the larger one, :597-605, and
	 * blz_spmv takes any pair of blocks).  Several ranks: a block lives on ONE side (side_of), and a rank's slab of the
	 * long side of a tall matrix is many times its slab of the short one (relat9 shape at N = 8: 1.5 M rows against
	 * 69 k) -- each block is sized by its own side (round 2 gave all four the larger: 23 x what V, AV and P need there). */
	for (int b = 0; b < 4; b++) {
		const int64_t rows = nranks == 1 ? std::max(c->stride[0], c->stride[1]) : c->stride[side_of(b)];
		const size_t bytes = (size_t)std::max<int64_t>(rows, 1) * c->cfg.n * c->cfg.word;
		if (c->slab[b])
			hipFree(c->slab[b]);
		c->slab[b] = nullptr;
		HIPCHK(hipMalloc(&c->slab[b], bytes));
		HIPCHK(hipMemset(c->slab[b], 0, bytes));		/* sequential/lanczos_modp.c:617-622 */
		c->slab_bytes[b] = bytes;
	}
	for (int sd = 0; sd < 2; sd++) {
		if (c->gath[sd])
			hipFree(c->gath[sd]);
		c->gath[sd] = nullptr;
		c->gath_holds[sd] = -1;
		/* side sd is gathered by the product whose rows live on the other side; in its short-side form nothing is */
		const int t_gath = c->row_side[0] == 1 - sd ? 0 : 1;
		if (nranks > 1 && !c->short_side[t_gath]) {
			const size_t gb = (size_t)std::max<int64_t>(c->stride[sd], 1) * nranks * c->cfg.n * c->cfg.word;
			HIPCHK(hipMalloc(&c->gath[sd], gb));
			HIPCHK(hipMemset(c->gath[sd], 0, gb));
		}
	}
	while ((int)c->ev_piece.size() < K) {
		hipEvent_t e;
		HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		c->ev_piece.push_back(e);
	}
	HIPCHK(hipMemset(c->ctl, 0, sizeof(DevCtl)));
	c->host_ctl = DevCtl{};
	{
		int rc_ = explicit_p_state(c);		/* p = 0 as it stands */
		if (rc_ != BLZ_OK)
			return rc_;
	}
	c->have_matrix = true;
	return BLZ_OK;
}

/* One rank, the product in one piece: what follows the upload of slab t = csr[t][0] (row_ptr: its row pointers on the host) */
static void slab_whole_choices(blz_ctx *c, int t, const u32 *row_ptr, int64_t cols, bool dot_slab, int nranks, bool uploaded)
{
	/* Gathers that mostly hit (a banded / well-ordered matrix: the locality rule of spmv_plan_staged): the product
	 * is paced by the kernel, and there the staged form with 16-byte lanes plus the inner products as their own
	 * matrix-core kernel beat the fused lane-per-column form -- band matrix, 2 M x 2 M, n = 8: 308 + 55 us against
	 * 389 (profiles/r03_band_switches.txt).  Where the fabric paces the gathers the fused form stays (the inner
	 * products ride along for 20 us). */
	DevCsr &D = c->csr[t][0];
	if (uploaded && dot_slab && nranks == 1 && !D.wide && block_dot_mfma_supported(c->cfg) && D.panel_rows == 0 &&
	    D.locality < 0.3 && !D.uneven && D.outlier_share < 0.02) {
		spmv_plan_staged(c->cfg, row_ptr, D, true);
		c->fuse_local_off = D.st_ok;
	}
	const char *xe = getenv("BLZ_XCD_RANGES");	/* 0 / 1 force it off / on (A/B) */
	/* (an operand of a few MB sits in every L2 anyway: nothing to separate) */
	const bool big = (double)cols * c->cfg.n * c->cfg.word > 8e6;
	c->csr[t][0].xcd_ranges = xe ? xe[0] == '1' : (c->locality[t] < 0.6 && big);
}

/* allow_short_side = false: plan no short-side product (a bordered context: the border rows of the operand are not
 * gathered in that form) */
static int set_matrix_prepared(blz_ctx *c, const blz_prepared *P, int rank, bool allow_short_side)
{
	if (!c || !P)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_prepared: NULL argument");
	const int nranks = P->nranks, right = P->right, K = P->chunks;
	if (rank < 0 || rank >= nranks)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix: rank %d of %d", rank, nranks);
	if (nranks > 1 && (unsigned __int128)nranks * c->prime > ((unsigned __int128)1 << 64))
		return blz_fail(BLZ_EINVAL, "nranks * p must not exceed 2**64 (u64 all-reduce of residues)");
	if (K > 1 && nranks == 1 && !c->force_comm)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_prepared: the matrix was prepared in %d pieces for a single rank", K);
	if (P->val_hi[0] || P->val_hi[1]) {
		if (K > 1)
			return blz_fail(BLZ_EINVAL, "blz_set_matrix_prepared: wide matrix entries need the products in one piece");
		const int rcw = wide_refuse_ranks(c, "blz_set_matrix_prepared", nranks);
		if (rcw != BLZ_OK)
			return rcw;
	}
	if (c->loop && (rank != c->loop_rank || nranks != c->loop->nranks))
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_prepared: rank %d of %d, but the context is rank %d of %d in its loopback communicator",
				rank, nranks, c->loop_rank, c->loop->nranks);
	HIPCHK(hipSetDevice(c->device));
	MatrixShape S = { right, rank, nranks, K, P->nrows, P->ncols, { P->bounds[0], P->bounds[1] }, { P->stride[0], P->stride[1] }, {},
			  { P->share[0], P->share[1] }, { P->locality[0], P->locality[1] }, P->order_kind };
	if (P->has_perm) {
		S.perm[0].assign(P->perm[0], P->perm[0] + P->nrows);
		S.perm[1].assign(P->perm[1], P->perm[1] + P->ncols);
	}
	matrix_begin(c, S);
	int rc = BLZ_OK;
	/* Short-side form of a product whose operand side is at least 8 times longer than its output side (64-bit words:
	 * the partial sums travel as u64).  BLZ_SHORT_SIDE=0 / 1 forces it off / on (tests, A/B). */
	size_t part_need = 0, rs_need = 0;
	for (int t = 0; t < 2; t++) {
		const int rs_t = c->row_side[t], cs_t = 1 - rs_t;
		bool on = (nranks > 1 || c->force_comm) && c->cfg.word == 8 && c->glob_rows[cs_t] >= 8 * c->glob_rows[rs_t];
		if (const char *e = getenv("BLZ_SHORT_SIDE"))
			on = e[0] == '1' && c->cfg.word == 8 && (nranks > 1 || c->force_comm);
		if (!allow_short_side)
			on = false;
		c->short_side[t] = on;
		if (on) {
			part_need = std::max(part_need, (size_t)nranks * (size_t)std::max<int64_t>(c->stride[rs_t], 1) * c->cfg.n * 8);
			rs_need = std::max(rs_need, (size_t)std::max<int64_t>(c->stride[rs_t], 1) * c->cfg.n * 8);
		}
	}
	for (int t = 0; t < 2 && rc == BLZ_OK; t++) {
		if (c->short_side[t]) {
			blz_csr sh;
			if ((rc = blz_prepared_slab_short(P, rank, t, &sh)) != BLZ_OK)
				break;
			rc = upload_csr(c, sh, c->csr_short[t]);
			blz_csr_free(&sh);
			continue;		/* the gathering form of this product is not uploaded at all */
		}
		blz_csr slab;
		memset(&slab, 0, sizeof slab);
		const bool dot_slab = carries_dots(c, t);
		const bool whole = nranks == 1;		/* one rank: the slab IS the prepared CSR, no copy */
		if (whole)
			slab = P->full[t];
		else if ((rc = blz_prepared_slab(P, rank, t, &slab)) != BLZ_OK)
			break;
		if (K == 1) {
			/* product t gathers block rows by the column index of its slab: columns of M for t = 0, rows of M for t = 1 */
			const int64_t hot_t = c->cfg.panel ? P->hot[t == 0 ? 1 : 0] : 0;
			rc = upload_csr(c, slab, c->csr[t][0], hot_t, dot_slab, nranks == 1 ? c->locality[t] : 1.0,
					whole ? P->val_hi[t] : nullptr);
			slab_whole_choices(c, t, slab.row_ptr, slab.cols, dot_slab, nranks, rc == BLZ_OK);
		} else {
			/* columns are positions in the gathered operand of the opposite side: piece k = [k*w, (k+1)*w) */
			const int csd = 1 - c->row_side[t];
			const int64_t width = (c->stride[csd] / K) * nranks;
			std::vector<blz_csr> piece((size_t)K);
			rc = blz_csr_split_columns(&slab, width, K, piece.data());
			for (int k = 0; k < K && rc == BLZ_OK; k++)
				rc = upload_csr(c, piece[(size_t)k], c->csr[t][(size_t)k], 0, dot_slab);
			for (auto &pc : piece)
				blz_csr_free(&pc);
		}
		if (!whole)
			blz_csr_free(&slab);
	}
	if (rc != BLZ_OK)
		return rc;

	if (part_need > c->part_bytes) {
		if (c->part)
			hipFree(c->part);
		c->part = nullptr;
		HIPCHK(hipMalloc(&c->part, part_need));
		c->part_bytes = part_need;
	}
	if (rs_need > c->rs_bytes) {
		if (c->rs_recv)
			hipFree(c->rs_recv);
		c->rs_recv = nullptr;
		HIPCHK(hipMalloc(&c->rs_recv, rs_need));
		c->rs_bytes = rs_need;
	}
	return matrix_blocks(c, nranks, K);
}

extern "C" int blz_set_matrix_prepared(blz_ctx *c, const blz_prepared *P, int rank)
{
	if (c && c->wide_hi)	/* (a prepared object was made without them: the matrix would be that of the low limbs alone) */
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_prepared: high limbs are pending (blz_set_values_wide); they go with "
				"blz_set_matrix, blz_set_matrix_rhs or blz_set_matrix_rhs_block");
	return set_matrix_prepared(c, P, rank, true);
}

/* The one-call form: prepare for this context, keep this rank's share, drop the rest.  Several contexts of one process
 * (or several processes on a node) should prepare ONCE and call blz_set_matrix_prepared instead. */
extern "C" int blz_set_matrix(blz_ctx *c, const blz_coo *M, int right, int rank, int nranks)
{
	if (!c || !M)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix: NULL argument");
	if (nranks < 1 || rank < 0 || rank >= nranks)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix: rank %d of %d", rank, nranks);
	blz_prepared *P = nullptr;
	int rc;
	/* Wide value mode: the pending high limbs belong to this matrix and are consumed here, whatever comes of the call
	 * (a call that fails leaves the context out of the mode: no matrix of it is resident or pending).  An ordinary matrix:
	 * the mode describes the matrix that is resident or about to be set. */
	const u32 *hi = c->wide_hi;
	c->wide_hi = nullptr;
	c->values_wide = false;
	blz_coo Mp = *M;	/* what the preparation runs on */
	std::vector<u32> number;
	if (hi) {
		const int64_t hn = c->wide_nnz;
		c->wide_nnz = 0;
		if ((rc = wide_refuse_ranks(c, "blz_set_matrix", nranks)) != BLZ_OK)
			return rc;
		if (hn != M->nnz)
			return blz_fail(BLZ_EINVAL, "blz_set_matrix: %lld high limbs for a matrix of %lld entries (blz_set_values_wide)",
					(long long)hn, (long long)M->nnz);
		if (M->nnz > 0xFFFFFFFFll)
			return blz_fail(BLZ_EINVAL, "blz_set_matrix: too many entries");
		for (int64_t k = 0; k < M->nnz; k++)
			if ((((uint64_t)hi[k] << 32) | M->x[k]) >= c->prime)
				return blz_fail(BLZ_EINVAL, "blz_set_matrix: entry %lld is not a residue below p (wide value mode)", (long long)k);
		bool any_hi = false;
		for (int64_t k = 0; k < M->nnz && !any_hi; k++)
			any_hi = hi[k] != 0;
		/* Every high limb zero: the ordinary path, value-dependent choices (a matrix of ones is a pattern) included -- the
		 * plans and the words are those of a context that was never given a high array.  Otherwise the whole preparation
		 * runs on the entry NUMBERS in place of the values; one gather at the end fills both limbs. */
		if (any_hi) {
			number.resize((size_t)M->nnz);
			for (int64_t k = 0; k < M->nnz; k++)
				number[(size_t)k] = (u32)k;
			Mp.x = number.data();
		}
	}
	if ((rc = blz_prepare_for(c, &Mp, right, nranks, &P)) != BLZ_OK)
		return rc;
	if (!number.empty())
		rc = blz_prepared_fill_wide(P, M->x, hi);
	if (rc == BLZ_OK)
		rc = blz_set_matrix_prepared(c, P, rank);
	blz_prepared_free(P);
	c->values_wide = hi && rc == BLZ_OK;
	return rc;
}

/* ---- right-hand sides: M x = b / x M = b as kernel vectors of the bordered operator [M | b] / [M ; b].  Every setter ends in
 * border_install; who delegates to whom is listed in DESIGN.md section 11.3 ---- */

static int put_words(blz_ctx *c, void *dst, const uint64_t *src, int64_t words);
static inline bool exchanging(const blz_ctx *c);
static int coll_allreduce_i32(blz_ctx *c, const void *send, void *recv, size_t words, hipStream_t st);

static int rhs_refuse_ranks(const blz_ctx *c, const char *who, bool matrix_is_set)
{
	/* (the one-call form sets its own one-rank matrix: what an earlier matrix was set for does not count) */
	if ((matrix_is_set && c->nranks > 1) || c->comm || c->loop || c->force_comm)
		return blz_fail(BLZ_EINVAL, "%s: a right-hand side needs a single rank without a communicator (the border row is not "
				"distributed: see DESIGN.md section 11)", who);
	return BLZ_OK;
}

static int rhs_block_refuse_k(const blz_ctx *c, const char *who, int k)
{
	if (k < 1 || k > c->un || k > BLZ_MAX_RHS)
		return blz_fail(BLZ_EINVAL, "%s: %d right-hand sides: between 1 and min(n = %d, BLZ_MAX_RHS = %d) are possible", who, k,
				c->un, BLZ_MAX_RHS);
	return BLZ_OK;
}

/* what the one-rank setters, host and device, ask of the resident matrix */
static int rhs_refuse_pieces(const blz_ctx *c, const char *who, int k)
{
	if (c->csr[0].size() != 1 || c->csr[1].size() != 1 || c->short_side[0] || c->short_side[1] || c->glob_rows[0] < k)
		return blz_fail(BLZ_EINVAL, "%s: the matrix was not set for a single rank in one piece", who);
	return BLZ_OK;
}

static inline int border_row_words(int k) { return k == 1 ? 1 : border_kp(k); }

/* the same triplets under a dimension raised by k: k empty rows (x M = b) / columns (M x = b) */
static blz_coo bordered_coo(const blz_coo *M, int right, int k)
{
	blz_coo Mb = *M;
	(right ? Mb.ncols : Mb.nrows) += k;
	return Mb;
}

/*
 * Where the k border rows live, and are the ones this rank owns empty?  rows[i] = the position of border row i in the operand
 * of side 0 (on one rank in one piece: its row in the solver's numbering), own[i] = its local row where this rank owns it, -1
 * elsewhere.  The product whose rows live on side 0 says whether a row is empty, piece by piece.  A refusal is written to `why`
 * and not returned (nothing is read once `why` holds one): the one-rank setters return it at once, blz_set_rhs_ranks behind its
 * collective.  What is returned is the same on every rank (bounds and strides are every rank's).  single: the wording of
 * the one-column setters.
 */
static int border_locate(blz_ctx *c, const char *who, int k, bool single, std::vector<int64_t> &rows, std::vector<int64_t> &own,
			 char *why, size_t why_len)
{
	const int K = (int)c->csr[0].size(), t0 = c->row_side[0] == 0 ? 0 : 1;
	const int64_t first = c->glob_rows[0] - k;
	rows.assign((size_t)k, 0);
	own.assign((size_t)k, -1);
	for (int i = 0; i < k; i++) {
		const int64_t row = c->perm[0].empty() ? first + i : c->perm[0][(size_t)(first + i)];
		int owner = 0;
		int64_t local = 0;
		const int64_t pos = blz_gathered_position(c->bounds[0].data(), c->nranks, c->stride[0], K, row, &owner, &local);
		if (pos < 0)
			return (int)pos;
		rows[(size_t)i] = pos;
		if (owner != c->rank)
			continue;
		own[(size_t)i] = local;
		for (int q = 0; q < K && !why[0]; q++) {
			const DevCsr &A = c->csr[t0][(size_t)q];
			u32 rp[2] = { 0, 1 };
			if (A.rows != c->count[0] || local >= A.rows ||
			    hipMemcpy(rp, A.row_ptr + local, sizeof rp, hipMemcpyDeviceToHost) != hipSuccess)
				snprintf(why, why_len, "%s: unexpected slab shape", who);
			else if (rp[0] != rp[1] && single)
				snprintf(why, why_len, "%s: the last %s of the matrix must be empty (it stands for the right-hand side)", who,
					 c->right ? "column" : "row");
			else if (rp[0] != rp[1])
				snprintf(why, why_len, "%s: the last %d %s of the matrix must be empty (they stand for the right-hand sides)",
					 who, k, c->right ? "columns" : "rows");
		}
	}
	return BLZ_OK;
}

/* the words the host setters upload: rows of border_row_words(k) words (allocated bare: blz_rhs_cut fills every one) */
struct BorderWords {
	std::unique_ptr<uint64_t[]> w;
	size_t count = 0;
};

/* bs = the rows [first, first + count) of side 1 (solver's numbering) of the len x k block b, border_row_words(k) words each;
 * a refusal (a word not below p) goes to `why` like border_locate's */
static void border_cut(blz_ctx *c, const char *who, int k, const uint64_t *b, int64_t first, int64_t count, BorderWords &bs,
		       char *why, size_t why_len)
{
	const int kw = border_row_words(k);
	if (why[0])
		return;
	bs.count = (size_t)std::max<int64_t>(count, 1) * kw;
	bs.w.reset(new uint64_t[bs.count]);
	if (blz_rhs_cut(b, c->glob_rows[1], k, kw, c->prime, c->perm[1].empty() ? nullptr : c->perm[1].data(), first, count,
			bs.w.get()) != BLZ_OK)
		snprintf(why, why_len, "%s: %s", who, blz_last_error());
}

/* everything of border_install that can fail: room for the partial rows of the border dot, the row tables on the device.  The
 * allocations come first, so that a border that is resident keeps tables of its own until all of them have succeeded. */
static hipError_t border_tables(blz_ctx *c, int k, const std::vector<int64_t> &rows, const std::vector<int64_t> *own)
{
	Border &B = c->bd;
	hipError_t e;
	long long tab[BLZ_MAX_RHS];
	const size_t need = (size_t)border_dot_max_blocks(c->cfg) * border_row_words(k) * BLZ_BORDER_MAXN;
	if (B.partial_words < need) {
		u64 *roomier = nullptr;
		if ((e = hipMalloc(&roomier, need * sizeof(u64))) != hipSuccess)
			return e;
		if (B.partial)
			hipFree(B.partial);
		B.partial = roomier;
		B.partial_words = need;
	}
	if (!B.rows_dev && (e = hipMalloc(&B.rows_dev, sizeof tab)) != hipSuccess)
		return e;
	if (own && !B.own_dev && (e = hipMalloc(&B.own_dev, sizeof tab)) != hipSuccess)
		return e;
	for (int i = 0; i < BLZ_MAX_RHS; i++)
		tab[i] = i < k ? rows[(size_t)i] : 0;
	if ((e = hipMemcpy(B.rows_dev, tab, sizeof tab, hipMemcpyHostToDevice)) != hipSuccess || !own)
		return e;
	for (int i = 0; i < BLZ_MAX_RHS; i++)
		tab[i] = i < k ? (*own)[(size_t)i] : -1;
	return hipMemcpy(B.own_dev, tab, sizeof tab, hipMemcpyHostToDevice);
}

/* The one way a border becomes resident.  rhs = a finished device buffer of border_row_words(k) words per row, which belongs to
 * the context from here on (freed if the call fails); rows, own = border_locate's, own = nullptr unless the border is
 * distributed.  The caller has drained the streams.  Everything that can fail comes before the swap: a failing call leaves
 * the border that was resident in place. */
static int border_install(blz_ctx *c, int k, const std::vector<int64_t> &rows, const std::vector<int64_t> *own, void *rhs)
{
	const hipError_t e = border_tables(c, k, rows, own);
	if (e != hipSuccess) {
		hipFree(rhs);
		return blz_fail(BLZ_EHIP, "border_install: %s", hipGetErrorString(e));
	}
	Border &B = c->bd;
	if (B.rhs)
		hipFree(B.rhs);
	B.rhs = rhs;
	B.k = k;
	B.row_words = border_row_words(k);
	B.rows = rows;
	B.distributed = own != nullptr;
	B.own = own ? *own : std::vector<int64_t>();
	/* the fused inner products would read the border rows of Av before the border dot has written them: the second product
	 * runs plain and block_dot as its own kernel */
	c->fuse_local_off = true;
	if (c->iter_graph) {
		hipGraphExecDestroy(c->iter_graph);
		c->iter_graph = nullptr;
	}
	return BLZ_OK;
}

/* border_install for the host setters: bs = border_cut's words, uploaded in the context's width */
static int border_install_host(blz_ctx *c, int k, const std::vector<int64_t> &rows, const std::vector<int64_t> *own,
			       const BorderWords &bs)
{
	void *rhs = nullptr;
	HIPCHK(hipMalloc(&rhs, bs.count * c->cfg.word));
	const int rc = put_words(c, rhs, bs.w.get(), (int64_t)bs.count);
	if (rc != BLZ_OK) {
		hipFree(rhs);
		return rc;
	}
	return border_install(c, k, rows, own, rhs);
}

/* the one-rank host setters past their own argument checks: blz_set_rhs (k = 1) and blz_set_rhs_block (k > 1), each under
 * its own name */
static int set_rhs_host(blz_ctx *c, const char *who, int k, const uint64_t *b)
{
	int rc = rhs_refuse_ranks(c, who, true);
	if (rc != BLZ_OK || (rc = rhs_refuse_pieces(c, who, k)) != BLZ_OK)
		return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	std::vector<int64_t> rows, own;
	BorderWords bs;
	char why[512] = "";
	if ((rc = border_locate(c, who, k, k == 1, rows, own, why, sizeof why)) != BLZ_OK)
		return rc;
	border_cut(c, who, k, b, 0, c->glob_rows[1], bs, why, sizeof why);
	if (why[0])
		return blz_fail(BLZ_EINVAL, "%s", why);
	return border_install_host(c, k, rows, nullptr, bs);
}

extern "C" int blz_set_rhs(blz_ctx *c, const uint64_t *b)
{
	if (!c || !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "no matrix loaded (blz_set_matrix)");
	HIPCHK(hipSetDevice(c->device));
	if (!b)
		return blz_fail(BLZ_EINVAL, "blz_set_rhs: b is NULL");
	return set_rhs_host(c, "blz_set_rhs", 1, b);
}

extern "C" int blz_set_matrix_rhs(blz_ctx *c, const blz_coo *M, int right, const uint64_t *b)
{
	if (!c || !M || !b)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_rhs: NULL argument");
	int rc = rhs_refuse_ranks(c, "blz_set_matrix_rhs", false);
	if (rc != BLZ_OK)
		return rc;
	const blz_coo Mb = bordered_coo(M, right, 1);
	if ((rc = blz_set_matrix(c, &Mb, right, 0, 1)) != BLZ_OK)
		return rc;
	return blz_set_rhs(c, b);
}

extern "C" int blz_has_rhs(const blz_ctx *c) { return c && c->have_matrix && c->bd.rhs != nullptr; }

extern "C" int blz_rhs_count(const blz_ctx *c) { return blz_has_rhs(c) ? c->bd.k : 0; }

extern "C" int blz_set_rhs_block(blz_ctx *c, int k, const uint64_t *b)
{
	if (!c || !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "no matrix loaded (blz_set_matrix)");
	HIPCHK(hipSetDevice(c->device));
	if (!b)
		return blz_fail(BLZ_EINVAL, "blz_set_rhs_block: b is NULL");
	int rc = rhs_block_refuse_k(c, "blz_set_rhs_block", k);
	if (rc != BLZ_OK)
		return rc;
	if (k == 1)
		return blz_set_rhs(c, b);	/* one column reports as blz_set_rhs */
	return set_rhs_host(c, "blz_set_rhs_block", k, b);
}

extern "C" int blz_set_matrix_rhs_block(blz_ctx *c, const blz_coo *M, int right, int k, const uint64_t *b)
{
	if (!c || !M || !b)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_rhs_block: NULL argument");
	int rc = rhs_block_refuse_k(c, "blz_set_matrix_rhs_block", k);
	if (rc != BLZ_OK || (rc = rhs_refuse_ranks(c, "blz_set_matrix_rhs_block", false)) != BLZ_OK)
		return rc;
	const blz_coo Mb = bordered_coo(M, right, k);
	if ((rc = blz_set_matrix(c, &Mb, right, 0, 1)) != BLZ_OK)
		return rc;
	return blz_set_rhs_block(c, k, b);
}

/* ---- the border on several ranks ---- */

extern "C" int blz_set_rhs_ranks(blz_ctx *c, int k, const uint64_t *b)
{
	if (!c || !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "no matrix loaded (blz_set_matrix)");
	HIPCHK(hipSetDevice(c->device));
	const bool plain = c->nranks == 1 && !c->comm && !c->loop && !c->force_comm;
	if (!b && plain)
		return blz_fail(BLZ_EINVAL, "blz_set_rhs_ranks: b is NULL");
	int rc = rhs_block_refuse_k(c, "blz_set_rhs_ranks", k);
	if (rc != BLZ_OK)
		return rc;
	if (plain)
		return blz_set_rhs_block(c, k, b);	/* a plain single rank: the one-rank border in every respect */
	/* the refusals below are the same on every rank (same k, same matrix, same mode): nobody is left alone in the collective
	 * further down.  What one rank alone may get wrong (a NULL b, a border row that is not empty) goes through it. */
	if (c->external_exchange)
		return blz_fail(BLZ_EINVAL, "blz_set_rhs_ranks: the context is in external-exchange mode (the all-reduce of the border "
				"words is the library's own)");
	if (c->short_side[0] || c->short_side[1])
		return blz_fail(BLZ_EINVAL, "blz_set_rhs_ranks: a product of this matrix runs in its short-side form, which a bordered "
				"context cannot use (the border rows of the operand are not gathered there): set the matrix with "
				"BLZ_SHORT_SIDE=0, or through blz_set_matrix_rhs_ranks");
	if (c->nranks > 1 && !c->comm && !c->loop)
		return blz_fail(BLZ_ECOMM, "nranks > 1 but blz_comm_init was not called");
	if (c->glob_rows[0] < k || c->csr[0].empty() || c->csr[0].size() != c->csr[1].size())
		return blz_fail(BLZ_EINVAL, "blz_set_rhs_ranks: unexpected matrix shape");
	HIPCHK(hipStreamSynchronize(c->stream));
	HIPCHK(hipStreamSynchronize(c->xstream));
	Border &B = c->bd;
	if (!B.send) {
		const size_t bytes = (size_t)BLZ_MAX_RHS * c->cfg.n * sizeof(u64);
		HIPCHK(hipMalloc(&B.send, bytes));
		HIPCHK(hipMalloc(&B.recv, bytes));
		HIPCHK(hipMemset(B.send, 0, bytes));
		HIPCHK(hipMemset(B.recv, 0, bytes));
	}
	std::vector<int64_t> gpos, own;
	BorderWords bs;
	char why[512] = "";
	if (!b)
		snprintf(why, sizeof why, "blz_set_rhs_ranks: b is NULL");
	if ((rc = border_locate(c, "blz_set_rhs_ranks", k, false, gpos, own, why, sizeof why)) != BLZ_OK)
		return rc;
	border_cut(c, "blz_set_rhs_ranks", k, b, c->first[1], c->count[1], bs, why, sizeof why);
	const int refuse = why[0] != 0;
	if (exchanging(c)) {	/* all ranks pass or all fail */
		int sum = 0;
		HIPCHK(hipMemcpy(B.send, &refuse, sizeof refuse, hipMemcpyHostToDevice));
		if ((rc = coll_allreduce_i32(c, B.send, B.recv, 1, c->stream)) != BLZ_OK)
			return rc;
		HIPCHK(hipStreamSynchronize(c->stream));
		HIPCHK(hipMemcpy(&sum, B.recv, sizeof sum, hipMemcpyDeviceToHost));
		if (sum && !refuse)
			return blz_fail(BLZ_EINVAL, "blz_set_rhs_ranks: refused on another rank (%d of %d): the border rows must be empty and "
					"every word of b below p", sum, c->nranks);
	}
	if (refuse)
		return blz_fail(BLZ_EINVAL, "%s", why);
	return border_install_host(c, k, gpos, &own, bs);
}

extern "C" int blz_set_matrix_rhs_ranks(blz_ctx *c, const blz_coo *M, int right, int k, const uint64_t *b, int rank, int nranks)
{
	if (!c || !M || !b)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_rhs_ranks: NULL argument");
	if (nranks < 1 || rank < 0 || rank >= nranks)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_rhs_ranks: rank %d of %d", rank, nranks);
	int rc = rhs_block_refuse_k(c, "blz_set_matrix_rhs_ranks", k);
	if (rc != BLZ_OK)
		return rc;
	if (nranks == 1 && !c->comm && !c->loop && !c->force_comm)
		return blz_set_matrix_rhs_block(c, M, right, k, b);
	if (c->wide_hi)		/* (pending high limbs on several ranks: set_values_wide refused the communicator, this refuses nranks) */
		return wide_refuse_ranks(c, "blz_set_matrix_rhs_ranks", nranks > 1 ? nranks : 2);
	if (c->external_exchange)
		return blz_fail(BLZ_EINVAL, "blz_set_matrix_rhs_ranks: the context is in external-exchange mode (the all-reduce of the "
				"border words is the library's own)");
	const blz_coo Mb = bordered_coo(M, right, k);
	blz_prepared *P = nullptr;
	if ((rc = blz_prepare_for(c, &Mb, right, nranks, &P)) != BLZ_OK)
		return rc;
	rc = set_matrix_prepared(c, P, rank, false);	/* no short-side product, whatever BLZ_SHORT_SIDE says */
	blz_prepared_free(P);
	if (rc != BLZ_OK)
		return rc;
	return blz_set_rhs_ranks(c, k, b);
}

extern "C" int64_t blz_rows(const blz_ctx *c, int block)
{
	return (c && block >= 0 && block < 4) ? c->glob_rows[side_of(block)] : -1;
}

extern "C" int64_t blz_local_rows(const blz_ctx *c, int block, int64_t *first)
{
	if (!c || block < 0 || block > 3)
		return -1;
	if (first)
		*first = c->first[side_of(block)];
	return c->count[side_of(block)];
}

extern "C" int64_t blz_local_nnz(const blz_ctx *c, int transpose)
{
	if (!c || !c->have_matrix)
		return -1;
	int64_t nnz = 0;
	if (c->short_side[transpose ? 1 : 0])
		return c->csr_short[transpose ? 1 : 0].nnz;
	for (const auto &A : c->csr[transpose ? 1 : 0])
		nnz += A.nnz;
	return nnz;
}

extern "C" int blz_locality(const blz_ctx *c, double locality[2], int *order_kind)
{
	if (!c || !c->have_matrix || !locality)
		return blz_fail(BLZ_EINVAL, "blz_locality: bad argument");
	locality[0] = c->locality[0];
	locality[1] = c->locality[1];
	if (order_kind)
		*order_kind = c->order_kind;
	return BLZ_OK;
}

extern "C" int64_t blz_panel_rows(const blz_ctx *c, int transpose, double *share)
{
	if (!c || !c->have_matrix)
		return -1;
	const int t = transpose ? 1 : 0;
	if (share)
		*share = c->hot_share[t == 0 ? 1 : 0];
	return c->csr[t].empty() ? 0 : c->csr[t][0].panel_rows;
}

/* does blz_iterate give the second product the inner products as its epilogue? (enqueue_iteration asks the same) */
static inline bool iteration_fuses(const blz_ctx *c)
{
	return c->fuse_dot && !c->fuse_local_off && spmv_dot_supported(c->cfg) && c->count[0] > 0 && !c->short_side[c->right];
}

/* Does the next blz_iterate take the self-dot path?  Both inner products are then products of a block with itself --
 * v^T Av = tmp^T tmp out of the first product, v^T A^2 v = Av^T Av out of the second -- and v is not read again.  One kernel
 * form (the streaming one, no outlier rows, whole rows per lane group) on one kind of context (one rank, no collectives, no
 * border, one piece per slab, no captured graph); every other case is enqueued as before. */
static inline bool selfdot_path(const blz_ctx *c)
{
	if (!c->selfdot || !c->partial_self || !c->have_matrix || !iteration_fuses(c) || exchanging(c) || c->nranks != 1 || c->bd.rhs
	    || c->use_graph || c->short_side[0] || c->short_side[1] || c->csr[0].size() != 1 || c->csr[1].size() != 1)
		return false;
	return spmv_self_ok(c->cfg, c->csr[!c->right][0], false, c->max_self_blocks)
	       && spmv_self_ok(c->cfg, c->csr[c->right][0], true, c->max_dot_blocks);
}

extern "C" int blz_selfdot_active(const blz_ctx *c) { return c && selfdot_path(c) ? 1 : 0; }

static void plan_launch(const SpmvGrids &g, blz_plan_launch *o)
{
	o->form = g.form == SPMV_FORM_PANEL ? BLZ_FORM_PANEL : (g.form == SPMV_FORM_STAGED ? BLZ_FORM_STAGED : BLZ_FORM_SPMV);
	o->xcd_ranges = g.xcd;
	o->split_log2 = g.split_log2;
	o->st_gathers = g.gathers;
	o->grid_stream = g.blocks;
	o->grid_heavy = g.hb;
	o->grid_combine = g.cb;
	o->grid_medium = g.mb;
}

extern "C" int blz_slab_plan(const blz_ctx *c, int transpose, int piece, blz_plan *out)
{
	if (!c || !out || !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "blz_slab_plan: no context, no matrix or out is NULL");
	const int t = transpose ? 1 : 0;
	const bool sh = c->short_side[t];
	if (piece < 0 || piece >= (sh ? 1 : (int)c->csr[t].size()))
		return blz_fail(BLZ_EINVAL, "blz_slab_plan: piece %d of %d", piece, sh ? 1 : (int)c->csr[t].size());
	const DevCsr &A = sh ? c->csr_short[t] : c->csr[t][(size_t)piece];
	memset(out, 0, sizeof *out);
	out->rows = A.rows;
	out->cols = A.cols;
	out->nnz = A.nnz;
	out->pieces = sh ? 1 : (int)c->csr[t].size();
	out->width = c->cfg.n;
	out->chunk = (int32_t)c->cfg.m.chunk;
	out->num_cu = c->cfg.num_cu;
	out->max_dot_blocks = c->max_dot_blocks;
	out->tail_batch = A.tail_batch;
	out->xcd_ranges = A.xcd_ranges;
	out->heavy_thr = A.heavy_thr;
	out->n_medium = A.n_medium;
	out->n_heavy = A.n_heavy;
	out->n_multi = A.n_multi;
	out->st_ok = A.st_ok;
	out->st_tr = A.st_tr;
	out->st_pair = A.st_pair;
	out->st_dyn = A.st_dyn;
	out->st_deep = A.st_deep;
	out->st_interleave = A.st_interleave;
	out->st_capw = A.st_capw;
	out->st_per_cu = A.st_per_cu;
	out->panel_rows = A.panel_rows;
	out->packed = A.palette ? 1 : (A.val ? 2 : 0);
	out->dot_supported = spmv_dot_supported(c->cfg);
	out->fuse_local_off = c->fuse_local_off;
	out->short_side = sh;
	out->locality = A.locality;
	plan_launch(spmv_grids(c->cfg, A, false, 0), &out->plain);
	if (out->dot_supported && !sh)
		plan_launch(spmv_grids(c->cfg, A, true, c->max_dot_blocks), &out->dot);
	/* the epilogue rides on the last piece of the second product */
	out->fused = t == (c->right ? 1 : 0) && iteration_fuses(c) && piece == out->pieces - 1;
	return BLZ_OK;
}

extern "C" int blz_slab_signed(const blz_ctx *c, int transpose, int piece)
{
	if (!c || !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "blz_slab_signed: no context or no matrix");
	const int t = transpose ? 1 : 0;
	const bool sh = c->short_side[t];
	if (piece < 0 || piece >= (sh ? 1 : (int)c->csr[t].size()))
		return blz_fail(BLZ_EINVAL, "blz_slab_signed: piece %d of %d", piece, sh ? 1 : (int)c->csr[t].size());
	const DevCsr &A = sh ? c->csr_short[t] : c->csr[t][(size_t)piece];
	return A.sgn ? 1 : 0;
}

extern "C" int blz_slab_wide(const blz_ctx *c, int transpose, int piece)
{
	if (!c || !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "blz_slab_wide: no context or no matrix");
	const int t = transpose ? 1 : 0;
	const bool sh = c->short_side[t];
	if (piece < 0 || piece >= (sh ? 1 : (int)c->csr[t].size()))
		return blz_fail(BLZ_EINVAL, "blz_slab_wide: piece %d of %d", piece, sh ? 1 : (int)c->csr[t].size());
	const DevCsr &A = sh ? c->csr_short[t] : c->csr[t][(size_t)piece];
	return A.wide ? 1 : 0;
}

extern "C" int64_t blz_matrix_stream_bytes(const blz_ctx *c, int transpose)
{
	if (!c || !c->have_matrix)
		return -1;
	int64_t bytes = 0;
	for (const auto &A : c->csr[transpose ? 1 : 0])
		bytes += (A.rows + 1) * 4 + A.nnz * 4 + (A.val ? A.nnz * 4 : 0) + (A.val_hi ? A.nnz * 4 : 0);
	return bytes;
}

/* host u64 words -> device words of the context's width */
static int put_words(blz_ctx *c, void *dst, const uint64_t *src, int64_t words)
{
	if (words <= 0)
		return BLZ_OK;
	if (c->cfg.word == 8) {
		HIPCHK(hipMemcpy(dst, src, (size_t)words * 8, hipMemcpyHostToDevice));
		return BLZ_OK;
	}
	std::vector<u32> tmp((size_t)words);
	for (int64_t k = 0; k < words; k++)
		tmp[(size_t)k] = (u32)src[k];
	HIPCHK(hipMemcpy(dst, tmp.data(), (size_t)words * 4, hipMemcpyHostToDevice));
	return BLZ_OK;
}

static int get_words(blz_ctx *c, uint64_t *dst, const void *src, int64_t words)
{
	if (words <= 0)
		return BLZ_OK;
	if (c->cfg.word == 8) {
		HIPCHK(hipMemcpy(dst, src, (size_t)words * 8, hipMemcpyDeviceToHost));
		return BLZ_OK;
	}
	std::vector<u32> tmp((size_t)words);
	HIPCHK(hipMemcpy(tmp.data(), src, (size_t)words * 4, hipMemcpyDeviceToHost));
	for (int64_t k = 0; k < words; k++)
		dst[k] = tmp[(size_t)k];
	return BLZ_OK;
}

/* `rows` block rows: host rows are c->un words wide, device rows c->cfg.n (zero-padded) */
static int put_rows(blz_ctx *c, void *dst, const uint64_t *src, int64_t rows)
{
	const int un = c->un, np = c->cfg.n;
	if (un == np || rows <= 0)
		return put_words(c, dst, src, rows * np);
	std::vector<uint64_t> wide((size_t)rows * np, 0);
	for (int64_t r = 0; r < rows; r++)
		memcpy(wide.data() + (size_t)r * np, src + (size_t)r * un, (size_t)un * sizeof(uint64_t));
	return put_words(c, dst, wide.data(), rows * np);
}

static int get_rows(blz_ctx *c, uint64_t *dst, const void *src, int64_t rows)
{
	const int un = c->un, np = c->cfg.n;
	if (un == np || rows <= 0)
		return get_words(c, dst, src, rows * np);
	std::vector<uint64_t> wide((size_t)rows * np);
	int rc = get_words(c, wide.data(), src, rows * np);
	for (int64_t r = 0; r < rows && rc == BLZ_OK; r++)
		memcpy(dst + (size_t)r * un, wide.data() + (size_t)r * np, (size_t)un * sizeof(uint64_t));
	return rc;
}

#define NEED_MATRIX(c)                                                                  \
	do {                                                                            \
		if (!(c) || !(c)->have_matrix)                                          \
			return blz_fail(BLZ_EINVAL, "no matrix loaded (blz_set_matrix)"); \
		HIPCHK(hipSetDevice((c)->device));                                      \
	} while (0)

extern "C" int blz_short_side(const blz_ctx *c, int transpose)
{
	return (c && c->have_matrix) ? (int)c->short_side[transpose ? 1 : 0] : -1;
}

/* the full-length partial product a short-side blz_spmv left behind (external-exchange mode: the caller does the
 * reduce-scatter): rows(dst side) x n words in the ORIGINAL numbering, sums not yet reduced mod p */
extern "C" int blz_get_partial(blz_ctx *c, int transpose, uint64_t *host)
{
	NEED_MATRIX(c);
	const int t = transpose ? 1 : 0;
	if (!host || !c->short_side[t])
		return blz_fail(BLZ_EINVAL, "blz_get_partial: product %d is not in the short-side form", t);
	HIPCHK(hipStreamSynchronize(c->stream));
	const int rs_t = c->row_side[t], np = c->cfg.n, un = c->un;
	std::vector<uint64_t> pad((size_t)c->nranks * c->stride[rs_t] * np);
	HIPCHK(hipMemcpy(pad.data(), c->part, pad.size() * 8, hipMemcpyDeviceToHost));
	for (int g = 0; g < c->nranks; g++)
		for (int64_t q = 0; q < c->bounds[rs_t][g + 1] - c->bounds[rs_t][g]; q++) {
			const int64_t solver_row = c->bounds[rs_t][g] + q;
			const int64_t orig = c->inv[rs_t].empty() ? solver_row : c->inv[rs_t][(size_t)solver_row];
			memcpy(host + (size_t)orig * un, pad.data() + ((size_t)g * c->stride[rs_t] + q) * np, (size_t)un * 8);
		}
	return BLZ_OK;
}

/* host block in ORIGINAL numbering -> one contiguous array in the solver's numbering (and back) */
static void to_solver_order(const blz_ctx *c, int sd, const uint64_t *host, uint64_t *out)
{
	const int n = c->un;
	const int64_t rows = c->glob_rows[sd];
	if (c->perm[sd].empty()) {
		memcpy(out, host, (size_t)rows * n * sizeof(uint64_t));
		return;
	}
	for (int64_t r = 0; r < rows; r++)
		memcpy(out + (size_t)c->perm[sd][(size_t)r] * n, host + (size_t)r * n, (size_t)n * sizeof(uint64_t));
}

extern "C" int blz_set_block(blz_ctx *c, int block, const uint64_t *host)
{
	NEED_MATRIX(c);
	if (block < 0 || block > 3 || !host)
		return blz_fail(BLZ_EINVAL, "blz_set_block: bad argument");
	HIPCHK(hipStreamSynchronize(c->stream));
	const int sd = side_of(block), n = c->un, np = c->cfg.n;
	std::vector<uint64_t> tmp;
	const uint64_t *src = host;
	if (!c->perm[sd].empty()) {
		tmp.resize((size_t)std::max<int64_t>(c->glob_rows[sd], 1) * n);
		to_solver_order(c, sd, host, tmp.data());
		src = tmp.data();
	}
	HIPCHK(hipStreamSynchronize(c->xstream));
	if (block == BLZ_P) {	/* p is what the caller says from here on */
		int rc_ = explicit_p_state(c);
		if (rc_ != BLZ_OK)
			return rc_;
	}
	/* this rank's rows */
	int rc = put_rows(c, c->slab[block], src + c->first[sd] * n, c->count[sd]);
	if (rc != BLZ_OK || c->nranks == 1 || !c->gath[sd])
		return rc;	/* (a side whose product runs in the short-side form has no gathered copy) */
	/* and, with several ranks, the whole gathered operand (an all-gather done by the caller): piece k of rank g
	 * sits at (k * nranks + g) * piece rows */
	const int K = (int)c->csr[0].size();
	const int64_t piece = c->stride[sd] / K;
	for (int g = 0; g < c->nranks; g++) {
		const int64_t b0 = c->bounds[sd][g], cnt = c->bounds[sd][g + 1] - b0;
		for (int k = 0; k < K; k++) {
			const int64_t q0 = (int64_t)k * piece, q1 = std::min<int64_t>(q0 + piece, cnt);
			if (q1 <= q0)
				break;
			char *dst = (char *)c->gath[sd] + (size_t)(((int64_t)k * c->nranks + g) * piece) * np * c->cfg.word;
			rc = put_rows(c, dst, src + (b0 + q0) * n, q1 - q0);
			if (rc != BLZ_OK)
				return rc;
		}
	}
	c->gath_holds[sd] = block;
	return BLZ_OK;
}

extern "C" int blz_get_block(blz_ctx *c, int block, uint64_t *host)
{
	NEED_MATRIX(c);
	if (block < 0 || block > 3 || !host)
		return blz_fail(BLZ_EINVAL, "blz_get_block: bad argument");
	if (block == BLZ_P) {
		int rc_ = materialize_p(c);
		if (rc_ != BLZ_OK)
			return rc_;
	}
	HIPCHK(hipStreamSynchronize(c->stream));
	HIPCHK(hipStreamSynchronize(c->xstream));
	const int sd = side_of(block), n = c->un;
	if (c->perm[sd].empty())
		return get_rows(c, host + c->first[sd] * n, slab_ptr(c, block), c->count[sd]);
	std::vector<uint64_t> tmp((size_t)std::max<int64_t>(c->count[sd], 1) * n);
	int rc = get_rows(c, tmp.data(), slab_ptr(c, block), c->count[sd]);
	if (rc != BLZ_OK)
		return rc;
	for (int64_t q = 0; q < c->count[sd]; q++)
		memcpy(host + (size_t)c->inv[sd][(size_t)(c->first[sd] + q)] * n, tmp.data() + (size_t)q * n,
		       (size_t)n * sizeof(uint64_t));
	return BLZ_OK;
}

extern "C" int blz_owner_of_row(const blz_ctx *c, int block, int64_t row)
{
	if (!c || !c->have_matrix || block < 0 || block > 3)
		return -1;
	const int sd = side_of(block);
	if (row < 0 || row >= c->glob_rows[sd])
		return -1;
	const int64_t r = c->perm[sd].empty() ? row : c->perm[sd][(size_t)row];
	int g = 0;
	while (g + 1 < c->nranks && c->bounds[sd][g + 1] <= r)
		g++;
	return g;
}

static int small_off(const blz_ctx *c, int which, int *words)
{
	const int nn = c->cfg.n * c->cfg.n;
	*words = which == BLZ_D ? c->cfg.n : nn;
	switch (which) {
	case BLZ_VTAV: return 0;
	case BLZ_VTAAV: return nn;
	case BLZ_WINV: return 2 * nn;
	case BLZ_D: return 3 * nn;
	default: return -1;
	}
}

extern "C" int blz_set_small(blz_ctx *c, int which, const uint64_t *host)
{
	if (!c || !host)
		return blz_fail(BLZ_EINVAL, "blz_set_small: NULL argument");
	HIPCHK(hipSetDevice(c->device));
	int words, off = small_off(c, which, &words);
	if (off < 0)
		return blz_fail(BLZ_EINVAL, "blz_set_small: unknown operand %d", which);
	HIPCHK(hipStreamSynchronize(c->stream));
	std::vector<u64> dev((size_t)words, 0);		/* the caller's un x un (or un) words inside the padded operand */
	const int un = c->un, np = c->cfg.n;
	if (which == BLZ_D)
		memcpy(dev.data(), host, (size_t)un * sizeof(u64));
	else
		for (int i = 0; i < un; i++)
			memcpy(dev.data() + (size_t)i * np, host + (size_t)i * un, (size_t)un * sizeof(u64));
	HIPCHK(hipMemcpy(c->small + off, dev.data(), (size_t)words * sizeof(u64), hipMemcpyHostToDevice));
	return BLZ_OK;
}

extern "C" int blz_get_small(blz_ctx *c, int which, uint64_t *host)
{
	if (!c || !host)
		return blz_fail(BLZ_EINVAL, "blz_get_small: NULL argument");
	HIPCHK(hipSetDevice(c->device));
	int words, off = small_off(c, which, &words);
	if (off < 0)
		return blz_fail(BLZ_EINVAL, "blz_get_small: unknown operand %d", which);
	HIPCHK(hipStreamSynchronize(c->stream));
	std::vector<u64> dev((size_t)words);
	HIPCHK(hipMemcpy(dev.data(), c->small + off, (size_t)words * sizeof(u64), hipMemcpyDeviceToHost));
	const int un = c->un, np = c->cfg.n;
	if (which == BLZ_D)
		memcpy(host, dev.data(), (size_t)un * sizeof(u64));
	else
		for (int i = 0; i < un; i++)
			memcpy(host + (size_t)i * un, dev.data() + (size_t)i * np, (size_t)un * sizeof(u64));
	return BLZ_OK;
}

extern "C" int blz_init_v(blz_ctx *c)
{
	NEED_MATRIX(c);
	HIPCHK(hipStreamSynchronize(c->stream));
	HIPCHK(hipStreamSynchronize(c->xstream));
	for (int b = 0; b < 4; b++)
		HIPCHK(hipMemset(c->slab[b], 0, c->slab_bytes[b]));
	c->gath_holds[0] = c->gath_holds[1] = -1;
	HIPCHK(hipMemset(c->ctl, 0, sizeof(DevCtl)));
	c->host_ctl = DevCtl{};
	{
		int rc_ = explicit_p_state(c);		/* p = 0 as it stands */
		if (rc_ != BLZ_OK)
			return rc_;
	}
	/* :624-625: one sequential stream over the whole block in ORIGINAL row order; a rank keeps the rows it owns. */
	const int n = c->un;
	const int64_t keep = c->count[0] * n, lo = c->first[0], hi = c->first[0] + c->count[0];
	std::vector<uint64_t> mine((size_t)std::max<int64_t>(keep, 1));
	uint64_t s[4];
	blz_rng_seed(s);
	for (int64_t r = 0; r < c->glob_rows[0]; r++) {
		const int64_t nr = c->perm[0].empty() ? r : c->perm[0][(size_t)r];
		if (nr >= lo && nr < hi) {
			for (int l = 0; l < n; l++)
				mine[(size_t)((nr - lo) * n + l)] = blz_rng_next(s) % c->prime;
		} else {
			for (int l = 0; l < n; l++)
				(void)blz_rng_next(s);
		}
	}
	return put_rows(c, slab_ptr(c, BLZ_V), mine.data(), c->count[0]);
}

/* ---- exchange steps (RCCL over xGMI).  No-ops on a single rank. ---- */

static inline bool exchanging(const blz_ctx *c)
{
	return !c->external_exchange && (c->nranks > 1 || (c->force_comm && (c->comm || c->loop)));
}

/* where k_dot_finalize puts this rank's sums: straight into `small` on one rank, into the send buffer otherwise */
static inline u64 *dot_out(blz_ctx *c);

/* ---- the four collectives of the solver, over RCCL or over the loopback group ---- */

enum { LOOP_GATHER = 0, LOOP_SUM64 = 1, LOOP_SUM64_SEGMENT = 2, LOOP_SUM32 = 3 };

/* one loopback collective of rank c->rank on stream st: `count` = bytes per rank (gather) or words (sums) */
static int loop_collective(blz_ctx *c, int kind, const void *send, void *recv, size_t count, hipStream_t st)
{
	blz_loop_group *g = c->loop;
	const int r = c->loop_rank, N = g->nranks;
	g->send[(size_t)r] = send;
	HIPCHK(hipEventRecord(g->ready[(size_t)r], st));
	if (!g->meet())
		return blz_fail(BLZ_ECOMM, "loopback communicator: a rank did not arrive (or gave up)");
	for (int q = 0; q < N; q++)
		if (q != r)
			HIPCHK(hipStreamWaitEvent(st, g->ready[(size_t)q], 0));
	if (kind == LOOP_GATHER) {
		for (int q = 0; q < N; q++)
			HIPCHK(launch_copy(c->cfg, (char *)recv + (size_t)q * count, g->send[(size_t)q], count, st));
	} else {
		const void *src[BLZ_LOOP_MAX_RANKS];
		for (int q = 0; q < N; q++)
			src[q] = kind == LOOP_SUM64_SEGMENT ? (const void *)((const u64 *)g->send[(size_t)q] + (size_t)r * count) : g->send[(size_t)q];
		HIPCHK(launch_sum_buffers(src, N, recv, (long long)count, kind == LOOP_SUM32 ? 4 : 8, st));
	}
	HIPCHK(hipEventRecord(g->done[(size_t)r], st));
	if (!g->meet())
		return blz_fail(BLZ_ECOMM, "loopback communicator: a rank did not arrive (or gave up)");
	for (int q = 0; q < N; q++)
		if (q != r)
			HIPCHK(hipStreamWaitEvent(st, g->done[(size_t)q], 0));
	return BLZ_OK;
}

static int coll_allgather(blz_ctx *c, const void *send, void *recv, size_t bytes, hipStream_t st)
{
	if (c->loop)
		return loop_collective(c, LOOP_GATHER, send, recv, bytes, st);
	if (!c->comm)
		return blz_fail(BLZ_ECOMM, "nranks > 1 but blz_comm_init was not called");
	NCCLCHK(g_rccl.AllGather(send, recv, bytes, ncclUint8, c->comm, st));
	return BLZ_OK;
}

static int coll_allreduce_u64(blz_ctx *c, const void *send, void *recv, size_t words, hipStream_t st)
{
	if (c->loop)
		return loop_collective(c, LOOP_SUM64, send, recv, words, st);
	if (!c->comm)
		return blz_fail(BLZ_ECOMM, "nranks > 1 but blz_comm_init was not called");
	NCCLCHK(g_rccl.AllReduce(send, recv, words, ncclUint64, ncclSum, c->comm, st));
	return BLZ_OK;
}

static int coll_allreduce_i32(blz_ctx *c, const void *send, void *recv, size_t words, hipStream_t st)
{
	if (c->loop)
		return loop_collective(c, LOOP_SUM32, send, recv, words, st);
	if (!c->comm)
		return blz_fail(BLZ_ECOMM, "nranks > 1 but blz_comm_init was not called");
	NCCLCHK(g_rccl.AllReduce(send, recv, words, ncclInt32, ncclSum, c->comm, st));
	return BLZ_OK;
}

/* recv[i] = sum over the ranks of send_q[rank * words + i] */
static int coll_reduce_scatter_u64(blz_ctx *c, const void *send, void *recv, size_t words, hipStream_t st)
{
	if (c->loop)
		return loop_collective(c, LOOP_SUM64_SEGMENT, send, recv, words, st);
	if (!c->comm)
		return blz_fail(BLZ_ECOMM, "nranks > 1 but blz_comm_init was not called");
	NCCLCHK(g_rccl.ReduceScatter(send, recv, words, ncclUint64, ncclSum, c->comm, st));
	return BLZ_OK;
}

static int allreduce_dots(blz_ctx *c)
{
	if (!exchanging(c))
		return BLZ_OK;
	Span sp(c, PK_AR);
	/* residues < p and nranks * p <= 2^64 (checked in blz_set_matrix): the u64 sum cannot wrap; the
	 * semi_inverse kernel reduces it mod p.  (mpi/lanczos_modp.c:1209-1247 does this by hand.)
	 * From the rank's own partial sums (dot_send) into a landing place of its own (dot_recv), never into `small`: the
	 * collective is enqueued by the host whatever the stop flag says, and the iterations a batch enqueues past the stop
	 * would leave raw sums (up to nranks * (p - 1)) in `small` -- the semi-inverse kernel, the one that turns them
	 * into residues, is a no-op by then.  It reads dot_recv and writes `small` only while the flag is down. */
	return coll_allreduce_u64(c, c->dot_send, c->dot_recv, (size_t)2 * c->cfg.n * c->cfg.n, c->stream);
}

static inline u64 *dot_out(blz_ctx *c) { return exchanging(c) ? c->dot_send : c->small; }

/* where the semi-inverse finds vtAv | vtAAv */
static inline const u64 *dot_sums(blz_ctx *c) { return exchanging(c) ? c->dot_recv : c->small; }

/*
 * The border of M' = [M | b] resp. [M ; b] behind product `transpose` (one rank; the matrix holds an empty row / column
 * in b's place).  The product that writes side 1 gets  dst[r, :] += b[r] * src[border, :],  the one that writes side 0
 *  dst[border, :] = sum_r b[r] * src[r, :]  (the SpMV has written zeros there).  Enqueued on the context's stream behind
 * launch_spmv, which has joined its outlier launches' side stream by the time it returns.
 */
static int enqueue_border(blz_ctx *c, int transpose, int src, int dst, const DevCtl *ctl, int cls)
{
	const Border &B = c->bd;
	const int k = B.k;
	const size_t last = (size_t)B.rows[(size_t)k - 1] * c->cfg.n * c->cfg.word;	/* k = 1: where the one border row starts */
	if (c->row_side[transpose] == 1) {
		/* The product that writes side 1 reads the k border rows of its operand: of the slab on one rank; on several, where
		 * the exchange has just put them (all K pieces have landed: the products above waited for them), at their positions
		 * in the gathered layout -- nothing more is exchanged. */
		Span sp(c, cls);
		const char *X = (const char *)operand_ptr(c, src);
		if (k > 1)	/* several right-hand sides: the same pass, fused over the k columns */
			HIPCHK(launch_border_update_k(c->cfg, slab_ptr(c, dst), B.rhs, X, B.rows_dev, k, c->count[1], ctl, c->stream));
		else
			HIPCHK(launch_border_update(c->cfg, slab_ptr(c, dst), B.rhs, X + last, c->count[1], ctl, c->stream));
		return BLZ_OK;
	}
	if (B.distributed && exchanging(c)) {
		/* Several ranks.  T and B are this rank's own rows.  The product that writes side 0 takes the dot over its own rows
		 * (zeros from a rank without any), all-reduces the k x n words and the owners store their rows.  The collective is
		 * enqueued whatever the stop flag says, out of a send buffer into a landing buffer of its own (the reasoning of
		 * allreduce_dots): past the stop the two kernels around it are no-ops and the slab keeps its rows. */
		{
			Span sp(c, cls);
			HIPCHK(launch_border_dot_send(c->cfg, slab_ptr(c, src), B.rhs, c->count[1], B.partial, B.send, k, ctl, c->stream));
		}
		{
			Span sp(c, PK_AR);
			int rc_ = coll_allreduce_u64(c, B.send, B.recv, (size_t)k * c->cfg.n, c->stream);
			if (rc_ != BLZ_OK)
				return rc_;
		}
		Span sp(c, cls);
		HIPCHK(launch_border_place(c->cfg, B.recv, slab_ptr(c, dst), B.own_dev, k, ctl, c->stream));
		return BLZ_OK;
	}
	Span sp(c, cls);
	if (k > 1)
		HIPCHK(launch_border_dot_k(c->cfg, slab_ptr(c, src), B.rhs, c->count[1], B.partial, slab_ptr(c, dst), B.rows_dev, k, ctl,
					   c->stream));
	else
		HIPCHK(launch_border_dot(c->cfg, slab_ptr(c, src), B.rhs, c->count[1], B.partial, slab_ptr(c, dst) + last, ctl, c->stream));
	return BLZ_OK;
}

/*
 * One product of the iteration: slab[dst] = (transpose ? M^T : M)[this rank's rows] * block `src`, with the
 * exchange of `src` pipelined against it.  The exchange stream all-gathers piece k of every rank's slab into
 * gath[side]; the compute stream waits for piece k only, then multiplies by csr[transpose][k] (entries whose
 * columns lie in piece k), accumulating into slab[dst] from the second piece on.  With K pieces the product hides
 * all but 1/K of itself behind the exchange; K = 1 is one all-gather followed by one product.
 * with_dot: the last piece carries block_dot_products as its epilogue (second product only); *nb = partial rows.
 */
static int enqueue_product(blz_ctx *c, int transpose, int src, int dst, bool with_dot, int *nb, const DevCtl *ctl = nullptr)
{
	if (!ctl)
		ctl = c->ctl;	/* (blz_solution runs its check past the stop, on control words of its own) */
	const bool xchg = exchanging(c);
	const int cls = transpose == !c->right ? PK_SPMV1 : PK_SPMV2;
	if (c->short_side[transpose]) {
		/* partial product of this rank's own rows of the operand, full length on the output side; reduce-scatter of the
		 * u64 sums; mod p.  Nothing is gathered. */
		const int rs_t = c->row_side[transpose];
		if (with_dot)
			return blz_fail(BLZ_EINVAL, "enqueue_product: the short-side form has no fused inner products");
		{
			Span sp(c, cls);
			HIPCHK(launch_spmv(c->cfg, c->csr_short[transpose], slab_ptr(c, src), c->part, 0, ctl, c->stream));
		}
		if (xchg) {
			{
				Span sp(c, PK_RS);
				int rc_ = coll_reduce_scatter_u64(c, c->part, c->rs_recv, (size_t)c->stride[rs_t] * c->cfg.n, c->stream);
				if (rc_ != BLZ_OK)
					return rc_;
			}
			/* out of place and stop-aware: past the stop `part` is stale (possibly the OTHER product's), the collective
			 * runs all the same, and slab[dst] must keep the last real product (blz_final_check reads TMP) */
			HIPCHK(launch_reduce_modp(c->cfg, c->slab[dst], c->rs_recv, c->count[rs_t] * c->cfg.n, ctl, c->stream));
		}
		return BLZ_OK;
	}
	const int K = (int)c->csr[transpose].size(), sd = side_of(src);
	if (xchg) {
		if (!c->comm && !c->loop)
			return blz_fail(BLZ_ECOMM, "nranks > 1 but blz_comm_init was not called");
		/* the exchange may start once everything enqueued so far (the producer of `src`, and every earlier
		 * reader of the gathered buffer it overwrites) has run */
		HIPCHK(hipEventRecord(c->ev_prod, c->stream));
		HIPCHK(hipStreamWaitEvent(c->xstream, c->ev_prod, 0));
		const size_t piece = (size_t)(c->stride[sd] / K) * c->cfg.n * c->cfg.word;
		char *recv = c->nranks == 1 ? (char *)c->slab[src] : (char *)c->gath[sd];	/* 1 rank: in place */
		for (int k = 0; k < K; k++) {
			{
				Span sp(c, src == BLZ_V ? PK_AG_V : PK_AG_T, c->xstream);
				int rc_ = coll_allgather(c, (char *)c->slab[src] + (size_t)k * piece, recv + (size_t)k * c->nranks * piece, piece,
							 c->xstream);
				if (rc_ != BLZ_OK)
					return rc_;
			}
			HIPCHK(hipEventRecord(c->ev_piece[(size_t)k], c->xstream));
		}
		c->gath_holds[sd] = src;
	} else if (c->nranks > 1 && c->gath_holds[sd] != src) {
		return blz_fail(BLZ_EINVAL, "external-exchange mode: block %d has not been gathered (blz_set_block)", src);
	}
	const void *X = operand_ptr(c, src);
	for (int k = 0; k < K; k++) {
		if (xchg)
			HIPCHK(hipStreamWaitEvent(c->stream, c->ev_piece[(size_t)k], 0));
		Span sp(c, cls);
		const DevCsr &A = c->csr[transpose][(size_t)k];
		if (with_dot && k == K - 1)
			HIPCHK(launch_spmv_dot(c->cfg, A, X, slab_ptr(c, dst), slab_ptr(c, BLZ_V), k > 0, c->partial,
					       c->max_dot_blocks, nb, ctl, c->stream));
		else
			HIPCHK(launch_spmv(c->cfg, A, X, slab_ptr(c, dst), k > 0, ctl, c->stream));
	}
	if (c->bd.rhs)
		return enqueue_border(c, transpose, src, dst, ctl, cls);
	return BLZ_OK;
}

static int enqueue_spmv(blz_ctx *c, int transpose, int src, int dst)
{
	return enqueue_product(c, transpose, src, dst, false, nullptr);
}

static int enqueue_dot(blz_ctx *c)
{
	int nb = 0;
	{
	Span sp(c, PK_DOT);
	HIPCHK(launch_block_dot(c->cfg, slab_ptr(c, BLZ_V), slab_ptr(c, BLZ_AV), c->count[0], c->partial,
				std::min(c->max_dot_blocks, c->cfg.num_cu * 8), &nb, c->ctl, c->stream));
	HIPCHK(launch_dot_finalize(c->cfg, c->partial, nb, dot_out(c), c->ctl, c->stream));
	}
	return allreduce_dots(c);
}

static int enqueue_ortho(blz_ctx *c, bool img_ready = false)
{
	Span sp(c, PK_ORTHO);
	HIPCHK(launch_orthogonalize(c->cfg, slab_ptr(c, BLZ_V), slab_ptr(c, BLZ_AV), slab_ptr(c, BLZ_P), c->count[0],
				    c->small, c->ctl, c->stream, img_ready));
	return BLZ_OK;
}

static int fetch_ctl(blz_ctx *c)
{
	HIPCHK(launch_publish_ctl(c->ctl, c->ctl_pinned_dev, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->host_ctl = *c->ctl_pinned;
	return BLZ_OK;
}

extern "C" int blz_spmv(blz_ctx *c, int transpose, int src_block, int dst_block)
{
	NEED_MATRIX(c);
	if (src_block < 0 || src_block > 3 || dst_block < 0 || dst_block > 3 || src_block == dst_block)
		return blz_fail(BLZ_EINVAL, "blz_spmv: bad block selectors");
	{	/* several ranks: a block lives on one side and its slab is sized for that side only */
		const int t = transpose ? 1 : 0;
		if (c->nranks > 1 && (side_of(dst_block) != c->row_side[t] || side_of(src_block) != 1 - c->row_side[t]))
			return blz_fail(BLZ_EINVAL, "blz_spmv: on several ranks product %d reads a block of side %d and writes one of side %d",
					t, 1 - c->row_side[t], c->row_side[t]);
	}
	int rc = (src_block == BLZ_P || dst_block == BLZ_P) ? materialize_p(c) : BLZ_OK;
	if (rc != BLZ_OK)
		return rc;
	rc = enqueue_spmv(c, transpose ? 1 : 0, src_block, dst_block);
	if (rc != BLZ_OK)
		return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	return BLZ_OK;
}

extern "C" int blz_block_dot(blz_ctx *c, uint64_t *vtAv, uint64_t *vtAAv)
{
	NEED_MATRIX(c);
	int rc = enqueue_dot(c);
	if (rc != BLZ_OK)
		return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	const int np = c->cfg.n, un = c->un, nn = np * np;
	std::vector<u64> h((size_t)2 * nn);
	if (exchanging(c)) {	/* the sums over the ranks -> residues in `small`, where a following blz_semi_inverse looks */
		HIPCHK(launch_reduce_modp(c->cfg, c->small, c->dot_recv, 2 * nn, c->ctl, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	HIPCHK(hipMemcpy(h.data(), c->small, (size_t)2 * nn * sizeof(u64), hipMemcpyDeviceToHost));
	for (int i = 0; i < un; i++) {
		if (vtAv)
			memcpy(vtAv + (size_t)i * un, h.data() + (size_t)i * np, (size_t)un * sizeof(u64));
		if (vtAAv)
			memcpy(vtAAv + (size_t)i * un, h.data() + nn + (size_t)i * np, (size_t)un * sizeof(u64));
	}
	return BLZ_OK;
}

extern "C" int blz_semi_inverse(blz_ctx *c, int *npiv, uint64_t *winv, uint64_t *d)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_semi_inverse: NULL context");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(launch_semi_inverse(c->cfg, c->small, c->small, c->ctl, 0, 0, c->stream));
	int rc = fetch_ctl(c);
	if (rc != BLZ_OK)
		return rc;
	if (npiv)
		*npiv = c->host_ctl.npiv;
	if (winv && (rc = blz_get_small(c, BLZ_WINV, winv)) != BLZ_OK)
		return rc;
	if (d && (rc = blz_get_small(c, BLZ_D, d)) != BLZ_OK)
		return rc;
	return BLZ_OK;
}

extern "C" int blz_orthogonalize(blz_ctx *c)
{
	NEED_MATRIX(c);
	int rc = materialize_p(c);	/* the stand-alone update is the explicit one, in place */
	if (rc != BLZ_OK)
		return rc;
	rc = enqueue_ortho(c);
	if (rc != BLZ_OK)
		return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	return BLZ_OK;
}

/* One pass of the loop body, sequential/lanczos_modp.c:635-656, enqueued on the stream. */
static int enqueue_iteration(blz_ctx *c)
{
	int rc;
	if (selfdot_path(c)) {
		/* :635, :636 and :640 in two kernels: each product leaves the inner product of its own output with itself */
		int nb1 = 0, nb2 = 0;
		{
			Span sp(c, PK_SPMV1);
			HIPCHK(launch_spmv_self(c->cfg, c->csr[!c->right][0], operand_ptr(c, BLZ_V), slab_ptr(c, BLZ_TMP), false,
						c->partial_self, c->max_self_blocks, &nb1, c->ctl, c->stream));
		}
		{
			Span sp(c, PK_SPMV2);
			HIPCHK(launch_spmv_self(c->cfg, c->csr[c->right][0], operand_ptr(c, BLZ_TMP), slab_ptr(c, BLZ_AV), true, c->partial,
						c->max_dot_blocks, &nb2, c->ctl, c->stream));
		}
		{
			Span sp(c, PK_DOT);
			HIPCHK(launch_dot_finalize_pair(c->cfg, c->partial_self, nb1, c->partial, nb2, c->small, c->ctl, c->stream));
		}
	} else if ((rc = enqueue_product(c, !c->right, BLZ_V, BLZ_TMP, false, nullptr)) != BLZ_OK) {	/* :635 */
		return rc;
	} else if (iteration_fuses(c)) {
		int nb = 0;							/* :636 + :640 in one kernel */
		if ((rc = enqueue_product(c, c->right, BLZ_TMP, BLZ_AV, true, &nb)) != BLZ_OK) return rc;
		{
			Span sp(c, PK_DOT);
			HIPCHK(launch_dot_finalize(c->cfg, c->partial, nb, dot_out(c), c->ctl, c->stream));
		}
		if ((rc = allreduce_dots(c)) != BLZ_OK) return rc;
	} else {
		if ((rc = enqueue_product(c, c->right, BLZ_TMP, BLZ_AV, false, nullptr)) != BLZ_OK) return rc;	/* :636 */
		if ((rc = enqueue_dot(c)) != BLZ_OK) return rc;				/* :640 */
	}
	/* the semi-inverse kernel also writes the coefficient image when the block update runs on the matrix cores
	 * (round 2: a launch of its own between the two) */
	const bool img = ortho_uses_mfma(c->cfg, c->count[0]);
	/* The rotating form (matrix-core update, no captured graph: a graph's launches have fixed arguments).  While every d[j]
	 * is non-zero -- every step but a few -- p' = v * winv does not depend on p, so it is not written: the update reads v,
	 * X and Av (p = X * E), writes v' into X's buffer, and the next step's (X, E) is (this v, untouched, winv).  When some
	 * d[j] = 0 the update also writes p' = X * (E (1 - D)) + v * winv into v's buffer and E <- I: at n = 8 out of the same
	 * image, at n = 16 after a pass that makes X = p first (a launch that returns at once on every other step).  Either way
	 * the two buffers have changed places: slab[BLZ_V] is v' for every later consumer. */
	const bool rot = img && !c->use_graph && !c->explicit_p;
	{
		Span sp(c, PK_SEMI);
		HIPCHK(launch_semi_inverse(c->cfg, dot_sums(c), c->small, c->ctl, 1, img, c->stream, rot ? c->un : 0));	/* :644 */
	}
	if (!rot)
		return enqueue_ortho(c, img);						/* :652-656 */
	const int np = c->cfg.n;
	Span sp(c, PK_ORTHO);
	if (np == 16)
		HIPCHK(launch_block_mul_gated(c->cfg, c->slab[BLZ_P], c->count[0], np, np, c->small + small_Emat(np), c->ctl,
					      c->small + small_materialize(np), c->stream));
	HIPCHK(launch_orthogonalize_rotate(c->cfg, slab_ptr(c, BLZ_V), slab_ptr(c, BLZ_AV), slab_ptr(c, BLZ_P), c->count[0],
					   c->small, c->ctl, c->stream));
	std::swap(c->slab[BLZ_V], c->slab[BLZ_P]);
	c->p_implicit = true;
	c->rot_swaps++;
	return BLZ_OK;
}

extern "C" int blz_iterate(blz_ctx *c, int max_iters, int *done, int *stopped, float *ms)
{
	NEED_MATRIX(c);
	if (max_iters < 0)
		return blz_fail(BLZ_EINVAL, "blz_iterate: max_iters < 0");
	if (c->external_exchange && c->nranks > 1)
		return blz_fail(BLZ_EINVAL, "blz_iterate: the context is in external-exchange mode");
	const long long before = c->host_ctl.iterations;
	c->rot_swaps = 0;
	HIPCHK(hipEventRecord(c->ev0, c->stream));
	const bool graph = c->use_graph && c->nranks == 1 && !c->force_comm && !c->profiling && max_iters > 1;
	if (graph && !c->iter_graph) {
		/* the loop body is a fixed sequence of launches with fixed arguments (all state lives in device memory):
		 * record it once, replay it per iteration */
		hipGraph_t g = nullptr;
		HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
		int rc = enqueue_iteration(c);
		hipError_t e = hipStreamEndCapture(c->stream, &g);
		if (rc != BLZ_OK)
			return rc;
		HIPCHK(e);
		HIPCHK(hipGraphInstantiate(&c->iter_graph, g, nullptr, nullptr, 0));
		hipGraphDestroy(g);
	}
	int enq_rc = BLZ_OK;
	for (int it = 0; it < max_iters; it++) {
		if (graph) {
			HIPCHK(hipGraphLaunch(c->iter_graph, c->stream));
			continue;
		}
		enq_rc = enqueue_iteration(c);
		if (enq_rc != BLZ_OK)
			break;		/* what was enqueued still runs: the swaps below are reconciled with it before the error goes out */
	}
	HIPCHK(hipEventRecord(c->ev1, c->stream));
	int rc = fetch_ctl(c);
	/* fetch_ctl fails on a device error only: how many steps ran is then unknown, the swaps below cannot be reconciled, and
	 * the context is unusable from here on (destroy it) */
	if (rc != BLZ_OK)
		return enq_rc != BLZ_OK ? enq_rc : rc;
	/* The rotating form swapped slab[BLZ_V] and slab[BLZ_P] once per ENQUEUED iteration, the device exchanged the roles of
	 * the two buffers once per iteration that RAN.  Invariant: ctl->iterations advances exactly when the block update runs
	 * (k_semi_inverse* increments it iff npiv > 0, and raises the stop flag otherwise, which turns the update and every
	 * later kernel of the batch into a no-op).  So (enqueued - run) swaps were one too many each: undo them, i.e. swap back
	 * once if that number is odd.  (A batch of the explicit form swapped nothing.) */
	if (c->rot_swaps > 0 && ((c->rot_swaps - (c->host_ctl.iterations - before)) & 1))
		std::swap(c->slab[BLZ_V], c->slab[BLZ_P]);
	if (enq_rc != BLZ_OK)
		return enq_rc;
	if (ms)
		HIPCHK(hipEventElapsedTime(ms, c->ev0, c->ev1));
	if (done)
		*done = (int)(c->host_ctl.iterations - before);
	if (stopped)
		*stopped = c->host_ctl.stop;
	return BLZ_OK;
}

extern "C" int64_t blz_iterations(const blz_ctx *c) { return c ? c->host_ctl.iterations : -1; }

extern "C" int blz_p_implicit(const blz_ctx *c) { return c && c->p_implicit ? 1 : 0; }

extern "C" int blz_set_iterations(blz_ctx *c, int64_t iterations)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_set_iterations: NULL context");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->host_ctl.iterations = iterations;
	HIPCHK(hipMemcpy(c->ctl, &c->host_ctl, sizeof(DevCtl), hipMemcpyHostToDevice));
	return BLZ_OK;
}

extern "C" int blz_final_check(blz_ctx *c, int *v_nonzero, int *vtm_zero)
{
	NEED_MATRIX(c);
	HIPCHK(hipStreamSynchronize(c->stream));
	HIPCHK(hipMemset(&c->ctl->flag_v_nonzero, 0, 2 * sizeof(int)));
	HIPCHK(launch_any_nonzero(c->cfg, slab_ptr(c, BLZ_V), c->count[0] * c->cfg.n, &c->ctl->flag_v_nonzero, c->stream));
	HIPCHK(launch_any_nonzero(c->cfg, slab_ptr(c, BLZ_TMP), c->count[1] * c->cfg.n, &c->ctl->flag_t_nonzero, c->stream));
	if (c->nranks > 1 && !c->external_exchange) {
		/* out of place (the sums land in dot_recv, idle at this point, and are copied back): the loopback communicator
		 * reads the other ranks' send buffers while they write their own results */
		int rc_ = coll_allreduce_i32(c, &c->ctl->flag_v_nonzero, c->dot_recv, 2, c->stream);
		if (rc_ != BLZ_OK)
			return rc_;
		HIPCHK(hipMemcpyAsync(&c->ctl->flag_v_nonzero, c->dot_recv, 2 * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
	}
	int rc = fetch_ctl(c);
	if (rc != BLZ_OK)
		return rc;
	if (v_nonzero)
		*v_nonzero = c->host_ctl.flag_v_nonzero != 0;
	if (vtm_zero)
		*vtm_zero = c->host_ctl.flag_t_nonzero == 0;
	return BLZ_OK;
}

/* ---- canonical RREF of a block's row space, and the kernel basis built on it ---- */

static int rref_alloc(blz_ctx *c)
{
	if (c->rref_ctl)
		return BLZ_OK;
	const size_t n = (size_t)c->un;
	HIPCHK(hipMalloc(&c->rref_stack, (size_t)c->cfg.num_cu * 2 * n * n * sizeof(u64)));
	HIPCHK(hipMalloc(&c->rref_gath, (size_t)c->nranks * n * n * sizeof(u64)));
	HIPCHK(hipMalloc(&c->rref_out, n * n * sizeof(u64)));
	HIPCHK(hipMalloc(&c->rref_z, n * n * sizeof(u64)));
	HIPCHK(hipMalloc(&c->rref_ctl, (3 + n) * sizeof(int)));
	return BLZ_OK;
}

/* RREF of `block` (this rank's rows, then, with several ranks, every rank's echelon merged) into rref_out / rref_ctl[2..] */
static int rref_to_host(blz_ctx *c, int block, uint64_t *E, int *rank, int32_t *pivots)
{
	int rc = rref_alloc(c);
	if (rc != BLZ_OK)
		return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	HIPCHK(hipStreamSynchronize(c->xstream));
	const int sd = side_of(block), n = c->un;
	HIPCHK(hipMemsetAsync(c->rref_ctl, 0, 2 * sizeof(int), c->stream));
	HIPCHK(launch_rref_partial(c->cfg, slab_ptr(c, block), c->count[sd], c->cfg.n, n, c->rref_stack, c->rref_ctl, c->stream));
	HIPCHK(launch_rref_merge(c->cfg, c->rref_stack, 0, c->rref_ctl + 1, n, c->rref_out, c->rref_ctl + 2, c->stream));
	if (c->nranks > 1 && !c->external_exchange) {
		/* every rank merges the same stack, so every rank holds the same RREF */
		rc = coll_allgather(c, c->rref_out, c->rref_gath, (size_t)n * n * sizeof(u64), c->stream);
		if (rc != BLZ_OK)
			return rc;
		HIPCHK(launch_rref_merge(c->cfg, c->rref_gath, (int64_t)c->nranks * n, nullptr, n, c->rref_out, c->rref_ctl + 2,
					 c->stream));
	}
	std::vector<int> info((size_t)n + 1);
	HIPCHK(hipMemcpyAsync(E, c->rref_out, (size_t)n * n * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(info.data(), c->rref_ctl + 2, info.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	*rank = info[0];
	for (int i = 0; i < n; i++)
		pivots[i] = info[(size_t)i + 1];
	return BLZ_OK;
}

extern "C" int blz_block_rref(blz_ctx *c, int block, uint64_t *rref, int *rank, int32_t *pivots)
{
	NEED_MATRIX(c);
	if (block < 0 || block > 3)
		return blz_fail(BLZ_EINVAL, "blz_block_rref: bad block %d", block);
	const int n = c->un;
	std::vector<uint64_t> E((size_t)n * n);
	std::vector<int32_t> piv((size_t)n);
	int r = 0;
	int rc = block == BLZ_P ? materialize_p(c) : BLZ_OK;
	if (rc != BLZ_OK)
		return rc;
	rc = rref_to_host(c, block, E.data(), &r, piv.data());
	if (rc != BLZ_OK)
		return rc;
	if (rref)
		memcpy(rref, E.data(), E.size() * sizeof(uint64_t));
	if (rank)
		*rank = r;
	if (pivots)
		memcpy(pivots, piv.data(), piv.size() * sizeof(int32_t));
	return BLZ_OK;
}

/* V <- V * Z (this rank's rows), Z = n x n host residues */
static int block_mul(blz_ctx *c, const std::vector<uint64_t> &Z)
{
	HIPCHK(hipMemcpyAsync(c->rref_z, Z.data(), Z.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
	HIPCHK(launch_block_mul(c->cfg, slab_ptr(c, BLZ_V), c->count[0], c->cfg.n, c->un, c->rref_z, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));	/* Z is a host vector */
	c->gath_holds[0] = -1;
	return BLZ_OK;
}

extern "C" int blz_kernel_basis(blz_ctx *c, int *k, uint64_t *z)
{
	NEED_MATRIX(c);
	const int n = c->un;
	const u64 p = c->prime;
	std::vector<uint64_t> E((size_t)n * n), Z0((size_t)n * n, 0), S((size_t)n * n, 0);
	std::vector<int32_t> piv((size_t)n);
	/* 1. E1 = RREF(TMP), rank s, pivots P */
	int s = 0;
	int rc = rref_to_host(c, BLZ_TMP, E.data(), &s, piv.data());
	if (rc != BLZ_OK)
		return rc;
	/* 2. Z0 = the canonical null basis of E1: one column per free column f, ascending: 1 at f, -E1[i][f] at pivot i */
	std::vector<char> is_piv((size_t)n, 0);
	for (int i = 0; i < s; i++)
		is_piv[(size_t)piv[(size_t)i]] = 1;
	int jj = 0;
	for (int f = 0; f < n; f++) {
		if (is_piv[(size_t)f])
			continue;
		Z0[(size_t)f * n + jj] = 1;
		for (int i = 0; i < s; i++)
			Z0[(size_t)piv[(size_t)i] * n + jj] = E[(size_t)i * n + f] ? p - E[(size_t)i * n + f] : 0;
		jj++;
	}
	/* 3. Y = V * Z0 (skipped when Z0 = I, i.e. s = 0) */
	if (s > 0 && (rc = block_mul(c, Z0)) != BLZ_OK)
		return rc;
	/* 4. E2 = RREF(Y): the basis is Y's columns at E2's pivots, moved to the front; the rest zeroed */
	int kk = 0;
	if ((rc = rref_to_host(c, BLZ_V, E.data(), &kk, piv.data())) != BLZ_OK)
		return rc;
	bool identity = kk == n;
	for (int i = 0; i < kk; i++) {
		S[(size_t)piv[(size_t)i] * n + i] = 1;
		identity &= piv[(size_t)i] == i;
	}
	if (!identity && (rc = block_mul(c, S)) != BLZ_OK)
		return rc;
	if (k)
		*k = kk;
	if (z)
		for (int row = 0; row < n; row++)
			for (int j = 0; j < n; j++)
				z[(size_t)row * n + j] = j < kk ? (s > 0 ? Z0[(size_t)row * n + piv[(size_t)j]] : (uint64_t)(row == piv[(size_t)j]))
								 : 0;
	return BLZ_OK;
}

/* a^-1 mod p (extended Euclid on the host, p prime, 0 < a < p) */
static uint64_t host_inverse(uint64_t a, uint64_t p)
{
	__int128 t = 0, nt = 1, r = p, nr = a % p;
	while (nr != 0) {
		const __int128 q = r / nr, t2 = t - q * nt, r2 = r - q * nr;
		t = nt;
		nt = t2;
		r = nr;
		nr = r2;
	}
	return (uint64_t)(t < 0 ? t + p : t);
}

/* the k border rows of V on the host, cfg.n words each.  Several ranks: every rank sends the rows it owns (zeros for the
 * others) through the border's all-reduce, so every rank reads the same words; collective. */
static int border_rows_to_host(blz_ctx *c, std::vector<uint64_t> &W)
{
	const Border &B = c->bd;
	const int np = c->cfg.n;
	W.assign((size_t)B.k * np, 0);
	if (B.distributed && exchanging(c)) {
		HIPCHK(launch_border_rows_send(c->cfg, slab_ptr(c, BLZ_V), B.own_dev, B.k, B.send, c->stream));
		int rc = coll_allreduce_u64(c, B.send, B.recv, (size_t)B.k * np, c->stream);
		if (rc != BLZ_OK)
			return rc;
		HIPCHK(hipStreamSynchronize(c->stream));
		HIPCHK(hipMemcpy(W.data(), B.recv, W.size() * sizeof(u64), hipMemcpyDeviceToHost));
		return BLZ_OK;
	}
	for (int i = 0; i < B.k; i++) {
		int rc = get_words(c, W.data() + (size_t)i * np, slab_ptr(c, BLZ_V) + (size_t)B.rows[(size_t)i] * np * c->cfg.word, np);
		if (rc != BLZ_OK)
			return rc;
	}
	return BLZ_OK;
}

/* does this rank hold row `orig` (original numbering) of side sd? */
static inline bool owns_row(const blz_ctx *c, int sd, int64_t orig)
{
	const int64_t r = c->perm[sd].empty() ? orig : c->perm[sd][(size_t)orig];
	return r >= c->first[sd] && r < c->first[sd] + c->count[sd];
}

/* the zero test of the verification product, summed over the ranks the way blz_final_check does it */
static int residual_flag(blz_ctx *c, int *nonzero)
{
	HIPCHK(hipMemsetAsync(&c->ctl->flag_t_nonzero, 0, sizeof(int), c->stream));
	HIPCHK(launch_any_nonzero(c->cfg, slab_ptr(c, BLZ_TMP), c->count[1] * c->cfg.n, &c->ctl->flag_t_nonzero, c->stream));
	if (c->nranks > 1 && !c->external_exchange) {
		int rc_ = coll_allreduce_i32(c, &c->ctl->flag_t_nonzero, c->dot_recv, 1, c->stream);
		if (rc_ != BLZ_OK)
			return rc_;
		HIPCHK(hipMemcpyAsync(&c->ctl->flag_t_nonzero, c->dot_recv, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
	}
	int rc = fetch_ctl(c);
	if (rc != BLZ_OK)
		return rc;
	*nonzero = c->host_ctl.flag_t_nonzero != 0;
	return BLZ_OK;
}

/* the side-1 product of V with the border applied, past the stop (on control words of its own), tested for zero on the
 * GPU like blz_final_check: *nonzero = some word of it is not zero */
static int solution_residual(blz_ctx *c, int *nonzero)
{
	DevCtl *idle = nullptr;
	HIPCHK(hipMalloc(&idle, sizeof(DevCtl)));
	hipError_t e = hipMemsetAsync(idle, 0, sizeof(DevCtl), c->stream);
	int rc = e == hipSuccess ? enqueue_product(c, !c->right, BLZ_V, BLZ_TMP, false, nullptr, idle) : BLZ_OK;
	if (e == hipSuccess)
		e = hipStreamSynchronize(c->stream);
	hipFree(idle);
	HIPCHK(e);
	if (rc != BLZ_OK)
		return rc;
	return residual_flag(c, nonzero);
}

static inline uint64_t host_mulmod(uint64_t a, uint64_t b, uint64_t p) { return (uint64_t)((unsigned __int128)a * b % p); }

/* What blz_solution_block and blz_solution_device share, everything but the way x leaves the slab: the kernel basis, the small
 * elimination on the host, V <- V * C and the verification product.  status[0..k) as blz_solution_block documents them;
 * *verified = the residual is zero, and then column i of V is (y_i, -e_i) where status[i] == 0 and zero where it is 1. */
static int solution_block_reduce(blz_ctx *c, int *status, bool *verified)
{
	*verified = false;
	const int n = c->un, np = c->cfg.n, k = c->bd.k;
	const u64 p = c->prime;
	int kb = 0;
	int rc = blz_kernel_basis(c, &kb, nullptr);
	if (rc != BLZ_OK)
		return rc;
	/* W = the k border rows of the kb basis vectors, next to -I_k: the basis vectors are v = (y, w) with M y + B w = 0, so a
	 * combination V c has border part W c, and W c = -e_i makes its upper part a solution of system i */
	const int cols = kb + k;
	std::vector<uint64_t> A((size_t)k * cols, 0), brow;
	if ((rc = border_rows_to_host(c, brow)) != BLZ_OK)
		return rc;
	for (int i = 0; i < k; i++) {
		for (int j = 0; j < kb; j++)
			A[(size_t)i * cols + j] = brow[(size_t)i * np + j];
		A[(size_t)i * cols + kb + i] = p - 1;
	}
	/* reduced row echelon form of [W | -I] over W's columns */
	std::vector<int> piv;
	int r = 0;
	for (int j = 0; j < kb && r < k; j++) {
		int q = r;
		while (q < k && A[(size_t)q * cols + j] == 0)
			q++;
		if (q == k)
			continue;
		for (int t = 0; t < cols && q != r; t++)
			std::swap(A[(size_t)q * cols + t], A[(size_t)r * cols + t]);
		const uint64_t inv = host_inverse(A[(size_t)r * cols + j], p);
		for (int t = 0; t < cols; t++)
			A[(size_t)r * cols + t] = host_mulmod(A[(size_t)r * cols + t], inv, p);
		for (int i = 0; i < k; i++) {
			const uint64_t f = A[(size_t)i * cols + j];
			if (i == r || f == 0)
				continue;
			for (int t = 0; t < cols; t++) {
				const uint64_t d = host_mulmod(f, A[(size_t)r * cols + t], p), a = A[(size_t)i * cols + t];
				A[(size_t)i * cols + t] = a >= d ? a - d : a + p - d;
			}
		}
		piv.push_back(j);
		r++;
	}
	/* system i is solved by this basis exactly when -e_i lies in W's column space: its reduced column is zero below the
	 * rank; then c = that column at the pivots, zero elsewhere */
	std::vector<uint64_t> Z((size_t)n * n, 0);
	for (int i = 0; i < k; i++) {
		status[i] = 0;
		for (int t = r; t < k; t++)
			if (A[(size_t)t * cols + kb + i])
				status[i] = 1;
		if (status[i])
			continue;
		for (int t = 0; t < r; t++)
			Z[(size_t)piv[(size_t)t] * n + i] = A[(size_t)t * cols + kb + i];
	}
	/* V <- V * C: column i = (y_i, -e_i), unsolved columns and the columns from k on zero */
	if ((rc = block_mul(c, Z)) != BLZ_OK)
		return rc;
	int nonzero = 0;
	if ((rc = solution_residual(c, &nonzero)) != BLZ_OK)
		return rc;
	if (nonzero) {
		for (int i = 0; i < k; i++)
			status[i] = 2;
		return BLZ_OK;
	}
	*verified = true;
	return BLZ_OK;
}

/* x <- the k solution columns of V without the border rows (the last k of the original numbering), the rows this rank owns
 * (several ranks: like blz_get_block) */
static int solution_to_host(blz_ctx *c, uint64_t *x)
{
	const int n = c->un, k = c->bd.k;
	std::vector<uint64_t> v((size_t)c->glob_rows[0] * n);
	int rc = blz_get_block(c, BLZ_V, v.data());
	if (rc != BLZ_OK)
		return rc;
	for (int64_t i = 0; i < c->glob_rows[0] - k; i++)
		for (int j = 0; j < k && owns_row(c, 0, i); j++)
			x[i * k + j] = v[(size_t)i * n + j];
	return BLZ_OK;
}

/* blz_solution_block on one column: with k = 1 the elimination of [W | -1] picks the first basis vector with a non-zero
 * border word w and scales it by -w^-1.  Its own argument checks, and x stays untouched unless the system is solved. */
extern "C" int blz_solution(blz_ctx *c, uint64_t *x, int *status)
{
	NEED_MATRIX(c);
	if (!c->bd.rhs || !x || !status)
		return blz_fail(BLZ_EINVAL, "blz_solution: %s", !c->bd.rhs ? "the context has no right-hand side (blz_set_matrix_rhs)" : "NULL argument");
	if (c->bd.k > 1)
		return blz_fail(BLZ_EINVAL, "blz_solution: the context has %d right-hand sides: use blz_solution_block", c->bd.k);
	bool verified = false;
	int rc = solution_block_reduce(c, status, &verified);
	if (rc != BLZ_OK || !verified || *status != 0)
		return rc;
	return solution_to_host(c, x);
}

extern "C" int blz_solution_block(blz_ctx *c, uint64_t *x, int *status)
{
	NEED_MATRIX(c);
	if (!c->bd.rhs || !x || !status)
		return blz_fail(BLZ_EINVAL, "blz_solution_block: %s",
				!c->bd.rhs ? "the context has no right-hand side (blz_set_matrix_rhs_block)" : "NULL argument");
	bool verified = false;
	int rc = solution_block_reduce(c, status, &verified);
	if (rc != BLZ_OK || !verified)
		return rc;
	return solution_to_host(c, x);
}

extern "C" int blz_time_kernel(blz_ctx *c, int which, int reps, float *ms_mean)
{
	NEED_MATRIX(c);
	if (reps < 1 || !ms_mean || which < 0 || which > 3)
		return blz_fail(BLZ_EINVAL, "blz_time_kernel: bad argument");
	if (which == 3) {	/* the explicit block update, in place on v and p */
		int rc = materialize_p(c);
		if (rc != BLZ_OK)
			return rc;
	}
	HIPCHK(hipEventRecord(c->ev0, c->stream));
	for (int r = 0; r < reps; r++) {
		int rc = BLZ_OK;
		switch (which) {
		case 0: rc = enqueue_spmv(c, !c->right, BLZ_V, BLZ_TMP); break;
		case 1: rc = enqueue_spmv(c, c->right, BLZ_TMP, BLZ_AV); break;
		case 2: rc = enqueue_dot(c); break;
		case 3: rc = enqueue_ortho(c); break;
		}
		if (rc != BLZ_OK)
			return rc;
	}
	HIPCHK(hipEventRecord(c->ev1, c->stream));
	HIPCHK(hipEventSynchronize(c->ev1));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
	*ms_mean = ms / reps;
	return BLZ_OK;
}

extern "C" int blz_profile(blz_ctx *c, int enable)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_profile: NULL context");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	for (auto &sp : c->spans) {
		c->pool.push_back(sp.a);
		c->pool.push_back(sp.b);
	}
	c->spans.clear();
	c->profiling = enable != 0;
	return BLZ_OK;
}

extern "C" int blz_profile_read(blz_ctx *c, double *ms_sum, int64_t *launches)
{
	if (!c || !ms_sum || !launches)
		return blz_fail(BLZ_EINVAL, "blz_profile_read: NULL argument");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	for (int k = 0; k < PK_COUNT; k++) {
		ms_sum[k] = 0;
		launches[k] = 0;
	}
	for (auto &sp : c->spans) {
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, sp.a, sp.b));
		ms_sum[sp.cls] += ms;
		launches[sp.cls] += 1;
	}
	return BLZ_OK;
}

/*
 * Asynchronous snapshot of (v, p, iteration count) for checkpoints -- openMP/lanczos_modp.c:1013-1022 stops the loop,
 * and round 1 did too (two synchronous blz_get_block calls and the file write on the loop thread).
 * blz_snapshot_begin: between two blz_iterate calls; copies this rank's rows of v and p device-to-device on the compute
 * stream (HBM speed), then enqueues the device-to-host copies of that snapshot into pinned staging on a stream of their
 * own and returns: the loop goes on while PCIe drains the snapshot (measured with a checkpoint every SECOND: 10.8 % loss on
 * the config-5 quarter shape when the loop waited for the 2 x 1.6 GB transfer, tools/exp_checkpoint.py).  If the two extra
 * slabs do not fit in HBM the copies read v and p directly and the compute stream waits for them.
 * blz_snapshot_wait: blocks until the copies have landed and unpacks this rank's rows into v / p (original numbering,
 * caller's width).  It touches only the snapshot's own staging and events, so it MAY be called from another host thread
 * (the checkpoint writer) while the owning thread is inside blz_iterate -- the one exception to one-thread-per-handle.
 */
extern "C" int blz_snapshot_begin(blz_ctx *c)
{
	NEED_MATRIX(c);
	if (c->snap_pending.load(std::memory_order_acquire))
		return blz_fail(BLZ_EINVAL, "blz_snapshot_begin: the previous snapshot has not been collected (blz_snapshot_wait)");
	if (!c->cstream) {
		HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
		HIPCHK(hipEventCreateWithFlags(&c->ev_snap_go, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&c->ev_snap_done, hipEventDisableTiming));
	}
	const size_t bytes = (size_t)std::max<int64_t>(c->count[0], 1) * c->cfg.n * c->cfg.word;
	if (bytes > c->snap_bytes) {
		for (int b = 0; b < 2; b++) {
			if (c->snap_host[b]) hipHostFree(c->snap_host[b]);
			if (c->snap_dev[b]) hipFree(c->snap_dev[b]);
			c->snap_host[b] = c->snap_dev[b] = nullptr;
			HIPCHK(hipHostMalloc(&c->snap_host[b], bytes, hipHostMallocDefault));
		}
		/* two more slabs of HBM let the PCIe transfer run beside the loop; without them the loop waits for it */
		if (hipMalloc(&c->snap_dev[0], bytes) != hipSuccess || hipMalloc(&c->snap_dev[1], bytes) != hipSuccess) {
			(void)hipGetLastError();
			for (void *&d : c->snap_dev) {
				if (d) hipFree(d);
				d = nullptr;
			}
		}
		c->snap_bytes = bytes;
	}
	{
		int rc = materialize_p(c);
		if (rc != BLZ_OK)
			return rc;
	}
	const bool staged = c->snap_dev[0] && c->snap_dev[1];
	if (staged) {
		/* device-to-device on the compute stream by a streaming kernel (2 x slab at HBM speed: 1.3 ms for 2 x 1.6 GB; the
		 * runtime's own device-to-device copy cost ~60 ms here), then the host copy reads
		 * the snapshot while later iterations overwrite v and p */
		HIPCHK(launch_copy(c->cfg, c->snap_dev[0], c->slab[BLZ_V], bytes, c->stream));
		HIPCHK(launch_copy(c->cfg, c->snap_dev[1], c->slab[BLZ_P], bytes, c->stream));
	}
	HIPCHK(hipEventRecord(c->ev_snap_go, c->stream));
	HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_snap_go, 0));
	HIPCHK(hipMemcpyAsync(c->snap_host[0], staged ? c->snap_dev[0] : c->slab[BLZ_V], bytes, hipMemcpyDeviceToHost, c->cstream));
	HIPCHK(hipMemcpyAsync(c->snap_host[1], staged ? c->snap_dev[1] : c->slab[BLZ_P], bytes, hipMemcpyDeviceToHost, c->cstream));
	HIPCHK(hipEventRecord(c->ev_snap_done, c->cstream));
	if (!staged)
		HIPCHK(hipStreamWaitEvent(c->stream, c->ev_snap_done, 0));	/* later kernels overwrite v and p in place */
	c->snap_iterations = c->host_ctl.iterations;
	c->snap_pending.store(true, std::memory_order_release);
	return BLZ_OK;
}

extern "C" int blz_snapshot_wait(blz_ctx *c, uint64_t *v, uint64_t *p, int64_t *iterations)
{
	if (!c || (!v) != (!p))
		return blz_fail(BLZ_EINVAL, "blz_snapshot_wait: NULL argument");
	if (!c->snap_pending.load(std::memory_order_acquire))
		return blz_fail(BLZ_EINVAL, "blz_snapshot_wait: no snapshot in flight");
	HIPCHK(hipSetDevice(c->device));
	/* polled, not hipEventSynchronize: this runs on the writer's thread while the owner keeps launching, and a blocking
	 * wait inside the runtime held the owner's launches back for the whole transfer (the loop lost as much time as if it
	 * had waited for the copy itself) */
	for (;;) {
		const hipError_t q = hipEventQuery(c->ev_snap_done);
		if (q == hipSuccess)
			break;
		if (q != hipErrorNotReady)
			return blz_fail(BLZ_EHIP, "blz_snapshot_wait: %s", hipGetErrorString(q));
		usleep(500);
	}
	const int un = c->un, np = c->cfg.n, sd = 0;
	uint64_t *dst[2] = { v, p };
	for (int b = 0; b < 2 && v; b++) {	/* v == p == NULL: the snapshot is dropped (a writer that failed elsewhere still collects) */
		const char *src = (const char *)c->snap_host[b];
		for (int64_t q = 0; q < c->count[sd]; q++) {
			const int64_t solver_row = c->first[sd] + q;
			const int64_t orig = c->inv[sd].empty() ? solver_row : c->inv[sd][(size_t)solver_row];
			uint64_t *out = dst[b] + (size_t)orig * un;
			if (c->cfg.word == 8) {
				memcpy(out, src + (size_t)q * np * 8, (size_t)un * 8);
			} else {
				const u32 *row = (const u32 *)(src + (size_t)q * np * 4);
				for (int l = 0; l < un; l++)
					out[l] = row[l];
			}
		}
	}
	if (iterations)
		*iterations = c->snap_iterations;
	c->snap_pending.store(false, std::memory_order_release);
	return BLZ_OK;
}

extern "C" int blz_sync(blz_ctx *c)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_sync: NULL context");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	HIPCHK(hipStreamSynchronize(c->xstream));
	return BLZ_OK;
}

extern "C" int blz_set_exchange_mode(blz_ctx *c, int external)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_set_exchange_mode: NULL context");
	if (external && c->have_matrix && c->bd.rhs && c->bd.distributed)
		return blz_fail(BLZ_EINVAL, "blz_set_exchange_mode: the context carries a right-hand side on several ranks (the all-reduce "
				"of its border words is the library's own)");
	if (external && c->device_ranks)
		return blz_fail(BLZ_EINVAL, "blz_set_exchange_mode: the context has device blocks on ranks switched on "
				"(blz_set_device_ranks), whose exchange is the library's own");
	c->external_exchange = external != 0;
	return BLZ_OK;
}

extern "C" int blz_comm_unique_id(void *id_out, size_t id_bytes)
{
	if (!id_out || id_bytes < sizeof(ncclUniqueId))
		return blz_fail(BLZ_EINVAL, "blz_comm_unique_id: need %zu bytes", sizeof(ncclUniqueId));
	int rc = rccl_load();
	if (rc != BLZ_OK)
		return rc;
	ncclUniqueId id;
	NCCLCHK(g_rccl.GetUniqueId(&id));
	memcpy(id_out, &id, sizeof id);
	return BLZ_OK;
}

extern "C" int blz_comm_init(blz_ctx *c, const void *id, size_t id_bytes, int rank, int nranks)
{
	if (!c || !id || id_bytes < sizeof(ncclUniqueId) || nranks < 1 || rank < 0 || rank >= nranks)
		return blz_fail(BLZ_EINVAL, "blz_comm_init: bad argument");
	if (c->values_wide)
		return blz_fail(BLZ_EINVAL, "blz_comm_init: the context is in wide value mode, which needs a single rank without a communicator");
	HIPCHK(hipSetDevice(c->device));
	int rc = rccl_load();
	if (rc != BLZ_OK)
		return rc;
	ncclUniqueId uid;
	memcpy(&uid, id, sizeof uid);
	NCCLCHK(g_rccl.CommInitRank(&c->comm, nranks, uid, rank));
	const char *f = getenv("BLZ_FORCE_COMM");
	c->force_comm = f && f[0] == '1';
	return BLZ_OK;
}

extern "C" int blz_comm_info(const blz_ctx *c, int *nranks_seen, int *rank_seen)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_comm_info: NULL context");
	int cnt = -1, rk = -1;
	if (c->loop) {
		cnt = c->loop->nranks;
		rk = c->loop_rank;
	} else if (c->comm) {
		NCCLCHK(g_rccl.CommCount(c->comm, &cnt));
		NCCLCHK(g_rccl.CommUserRank(c->comm, &rk));
	}
	if (nranks_seen)
		*nranks_seen = cnt;
	if (rank_seen)
		*rank_seen = rk;
	return BLZ_OK;
}

extern "C" int blz_exchange_pieces(const blz_ctx *c, int transpose)
{
	if (!c || !c->have_matrix)
		return -1;
	const int t = transpose ? 1 : 0;
	return c->short_side[t] ? 0 : (int)c->csr[t].size();
}

extern "C" int blz_exchange_pieces_for(const blz_ctx *c, int64_t mrows, int64_t mcols, int64_t nnz, int nranks)
{
	if (!c || nranks < 1)
		return -1;
	return prep_params(c, mrows, mcols, nnz, nranks).K;
}

/* ---- loopback communicator: several contexts of one process on one device (tests of the multi-rank path on one GPU) ---- */

extern "C" int blz_loop_group_create(int nranks, blz_loop_group **out)
{
	if (!out || nranks < 1 || nranks > BLZ_LOOP_MAX_RANKS)
		return blz_fail(BLZ_EINVAL, "blz_loop_group_create: 1 .. %d ranks", BLZ_LOOP_MAX_RANKS);
	blz_loop_group *g = new blz_loop_group();
	g->nranks = nranks;
	if (const char *e = getenv("BLZ_LOOP_TIMEOUT_S"))
		if (atoi(e) >= 1)
			g->timeout_s = atoi(e);
	g->send.assign((size_t)nranks, nullptr);
	g->ready.assign((size_t)nranks, nullptr);
	g->done.assign((size_t)nranks, nullptr);
	*out = g;
	return BLZ_OK;
}

extern "C" void blz_loop_group_destroy(blz_loop_group *g)
{
	if (!g)
		return;
	(void)hipDeviceSynchronize();
	for (hipEvent_t e : g->ready)
		if (e) hipEventDestroy(e);
	for (hipEvent_t e : g->done)
		if (e) hipEventDestroy(e);
	delete g;
}

extern "C" int blz_comm_init_loopback(blz_ctx *c, blz_loop_group *g, int rank)
{
	if (!c || !g || rank < 0 || rank >= g->nranks)
		return blz_fail(BLZ_EINVAL, "blz_comm_init_loopback: bad argument");
	if (c->values_wide)
		return blz_fail(BLZ_EINVAL, "blz_comm_init_loopback: the context is in wide value mode, which needs a single rank without a communicator");
	if (c->comm || c->loop)
		return blz_fail(BLZ_EINVAL, "blz_comm_init_loopback: the context has a communicator already");
	HIPCHK(hipSetDevice(c->device));
	{
		std::lock_guard<std::mutex> lk(g->mu);
		if (g->ready[(size_t)rank])
			return blz_fail(BLZ_EINVAL, "blz_comm_init_loopback: rank %d of the group is taken", rank);
		HIPCHK(hipEventCreateWithFlags(&g->ready[(size_t)rank], hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&g->done[(size_t)rank], hipEventDisableTiming));
	}
	c->loop = g;
	c->loop_rank = rank;
	c->rank = rank;
	const char *f = getenv("BLZ_FORCE_COMM");
	c->force_comm = f && f[0] == '1';
	return BLZ_OK;
}

/* ---- device blocks: set, get and apply M on caller-owned device memory (kernels: blz_devio.hip) ---- */

/* what belongs to the resident matrix: the scratch slabs of blz_apply_device, their control words, the numbering on the device */
static void devio_release_matrix(blz_ctx *c)
{
	if (c->stream && (c->slab[APPLY_SLAB] || c->slab[APPLY_SLAB + 1] || c->apply_ctl || c->inv_ready))
		hipStreamSynchronize(c->stream);	/* a product or a pass enqueued by the last call may still be running */
	for (int sd = 0; sd < 2; sd++) {
		if (c->slab[APPLY_SLAB + sd])
			hipFree(c->slab[APPLY_SLAB + sd]);
		c->slab[APPLY_SLAB + sd] = nullptr;
		c->slab_bytes[APPLY_SLAB + sd] = 0;
		if (c->inv_dev[sd])
			hipFree(c->inv_dev[sd]);
		c->inv_dev[sd] = nullptr;
	}
	c->inv_ready = false;
	if (c->apply_ctl)
		hipFree(c->apply_ctl);
	c->apply_ctl = nullptr;
}

static int devio_refuse_ranks(const blz_ctx *c, const char *who)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "%s: NULL context", who);
	if (c->device_ranks) {	/* blocks are rank-local: ranks are welcome, the caller's own exchange is not */
		if (c->external_exchange)
			return blz_fail(BLZ_EINVAL, "%s: device blocks on ranks need the library's own exchange, and the context is in "
					"external-exchange mode (blz_set_exchange_mode)", who);
		return BLZ_OK;
	}
	if (c->nranks > 1 || c->comm || c->loop || c->force_comm)
		return blz_fail(BLZ_EINVAL, "%s: device blocks need a single rank without a communicator, a loopback group or "
				"BLZ_FORCE_COMM (see DESIGN.md section 15)", who);
	return BLZ_OK;
}

/* ---- device blocks on ranks (kernels: blz_devrank.hip).  With blz_set_device_ranks a block of the
 * device-block family is the rank's own rows, count[side] of them, in slab order: import and export are the identity, the
 * products are enqueue_product with its exchange, an inner product ends in an all-reduce.  Every refusal below is a function
 * of what all ranks share (the mode, the matrix' shape and partition, the communicator's size, p), so either every rank
 * passes or every rank refuses, before the first enqueue and before any rendezvous. ---- */

extern "C" int blz_set_device_ranks(blz_ctx *c, int on)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_set_device_ranks: NULL context");
	c->device_ranks = on != 0;
	return BLZ_OK;
}

extern "C" int blz_device_ranks(const blz_ctx *c) { return c && c->device_ranks ? 1 : 0; }

extern "C" int blz_local_row_ids(const blz_ctx *c, int block, int64_t *ids)
{
	if (!c || !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "no matrix loaded (blz_set_matrix)");
	if (block < 0 || block > 3)
		return blz_fail(BLZ_EINVAL, "blz_local_row_ids: block %d is not one of V, TMP, AV, P", block);
	const int sd = side_of(block);
	if (!ids && c->count[sd] > 0)
		return blz_fail(BLZ_EINVAL, "blz_local_row_ids: ids is NULL");
	for (int64_t q = 0; q < c->count[sd]; q++)
		ids[q] = c->inv[sd].empty() ? c->first[sd] + q : (int64_t)c->inv[sd][(size_t)(c->first[sd] + q)];
	return BLZ_OK;
}

/* rows of a block of side sd as the device-block family sees it: the rank's own with the mode on, all of them otherwise
 * (the same number on one rank) */
static inline int64_t devio_rows(const blz_ctx *c, int sd) { return c->device_ranks ? c->count[sd] : c->glob_rows[sd]; }

/* the numbering an import / export goes through: none with the mode on (slab order) */
static inline const int32_t *devio_inv(const blz_ctx *c, int sd) { return c->device_ranks ? nullptr : c->inv_dev[sd]; }

/* a product of a mode-on context, before anything is enqueued: its short-side form has no scratch slab to run in, and an
 * exchange needs its communicator */
static int devrank_refuse_product(const blz_ctx *c, const char *who, int t)
{
	if (!c->device_ranks)
		return BLZ_OK;
	if (c->short_side[t])
		return blz_fail(BLZ_EINVAL, "%s: product %d of this matrix runs in the short-side form (blz_short_side), which device "
				"blocks on ranks do not have", who, t);
	if (c->nranks > 1 && !c->comm && !c->loop)
		return blz_fail(BLZ_ECOMM, "%s: nranks > 1 but blz_comm_init was not called", who);
	return BLZ_OK;
}

/* An error inside a collective device call, after the checks: the peers are at, or on their way to, a rendezvous this rank
 * will not reach.  Mark the loopback group broken so that they return BLZ_ECOMM at once, not after BLZ_LOOP_TIMEOUT_S.
 * (Mode-on calls only: nothing else changes what it does on an error.) */
static int devrank_collective_exit(blz_ctx *c, int rc)
{
	if (rc != BLZ_OK && c->device_ranks && c->loop) {
		std::lock_guard<std::mutex> lk(c->loop->mu);
		c->loop->broken = true;
		c->loop->cv.notify_all();
	}
	return rc;
}

/* ranks of the context's communicator (1 without one): the ranks of a collective dot, which needs no matrix */
static int devrank_comm_ranks(const blz_ctx *c, int *out)
{
	int cnt = 1;
	if (c->loop)
		cnt = c->loop->nranks;
	else if (c->comm)
		NCCLCHK(g_rccl.CommCount(c->comm, &cnt));
	*out = cnt;
	return BLZ_OK;
}

/* Is this dot collective, and may it be?  *N = the ranks its sum runs over (1: today's path, straight into c).  Checked
 * before anything is enqueued: nranks * p <= 2^64 (blz_set_matrix's rule: the u64 sum of the ranks' residues must not wrap). */
static int devrank_dot_ranks(const blz_ctx *c, const char *who, int *N, bool *collective)
{
	*N = 1;
	*collective = false;
	if (!c->device_ranks)
		return BLZ_OK;
	int rc = devrank_comm_ranks(c, N);
	if (rc != BLZ_OK)
		return rc;
	if (c->have_matrix && c->nranks > 1 && !c->comm && !c->loop)
		return blz_fail(BLZ_ECOMM, "%s: nranks > 1 but blz_comm_init was not called", who);
	*collective = (c->comm || c->loop) && (*N > 1 || c->force_comm);
	if (*collective && (unsigned __int128)*N * c->prime > ((unsigned __int128)1 << 64))
		return blz_fail(BLZ_EINVAL, "%s: nranks * p must not exceed 2**64 (u64 all-reduce of residues): %d ranks", who, *N);
	return BLZ_OK;
}

/* the tail of a collective dot on the context's stream: `words` residues of this rank in devrank_send -> all-reduce ->
 * their sums' residues in out */
static int devrank_dot_finish(blz_ctx *c, uint64_t *out, int words)
{
	int rc;
	{
		Span sp(c, PK_AR);
		rc = coll_allreduce_u64(c, c->devrank_send, c->devrank_recv, (size_t)words, c->stream);
	}
	if (rc != BLZ_OK)
		return rc;
	HIPCHK(launch_residue_sums(c->cfg, out, c->devrank_recv, words, c->stream));
	return BLZ_OK;
}

static int devrank_dot_buffers(blz_ctx *c)
{
	const size_t bytes = (size_t)2 * c->un * c->un * sizeof(u64);
	if (!c->devrank_send)
		HIPCHK(hipMalloc((void **)&c->devrank_send, bytes));
	if (!c->devrank_recv)
		HIPCHK(hipMalloc((void **)&c->devrank_recv, bytes));
	return BLZ_OK;
}

/* the look-up the two checks below share: `bytes` from ptr on lie inside ONE allocation of the context's device */
static int devio_check_alloc(const blz_ctx *c, const char *who, const char *arg, const void *ptr, size_t bytes, int64_t rows,
			     int64_t ld, int width = 0)	/* (width: the k words per row of a right-hand side or a solution) */
{
	hipPointerAttribute_t at;
	memset(&at, 0, sizeof at);
	if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
		(void)hipGetLastError();	/* (a plain host pointer is an error of the query on some runtimes, an unregistered type on others) */
		return blz_fail(BLZ_EINVAL, "%s: %s = %p is not device memory (a host pointer?)", who, arg, ptr);
	}
	if (at.type != hipMemoryTypeDevice)
		return blz_fail(BLZ_EINVAL, "%s: %s = %p is not device memory (memory type %d; a host pointer?)", who, arg, ptr, (int)at.type);
	if (at.device != c->device)
		return blz_fail(BLZ_EINVAL, "%s: %s lives on device %d, the context on device %d", who, arg, at.device, c->device);
	hipDeviceptr_t base = nullptr;
	size_t size = 0;
	if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) != hipSuccess || !base) {
		(void)hipGetLastError();
		return blz_fail(BLZ_EINVAL, "%s: the allocation of %s = %p cannot be found", who, arg, ptr);
	}
	const size_t off = (size_t)((const char *)ptr - (const char *)base);
	if (off > size || bytes > size - off)
		return blz_fail(BLZ_EINVAL, "%s: %s needs %zu bytes (%lld rows, row stride %lld, %s = %d) but its allocation ends after %zu",
				who, arg, bytes, (long long)rows, (long long)ld, width > 0 ? "k" : "n", width > 0 ? width : c->un,
				off > size ? (size_t)0 : size - off);
	return BLZ_OK;
}

/* No kernel is launched on memory the library has not checked: the words [ptr, ptr + ((rows - 1) * ld + n) * word) must lie
 * inside ONE allocation of the context's device, `word` being the bytes of a word of the caller's block (8, or 4 for the
 * 32-bit family).  A host pointer, another device's memory, managed or pinned host memory, a range that runs past its
 * allocation and ld < n are all BLZ_EINVAL, named by argument.  *bytes_out = the size checked.
 * `rows` is the block's own: a side of the matrix for set / get / apply, the caller's for the block algebra (an n x n operand
 * is n rows of stride n).  A block of no rows has no words: any pointer will do, nothing is looked up and *bytes_out = 0.
 * The size limits are each width's own: rows and stride at most 2^40 for 8-byte words, the byte count at most 2^62 for 4-byte
 * ones (whose callers have refused a negative row count before they come here). */
static int devio_check_range(const blz_ctx *c, const char *who, const char *arg, const void *ptr, int64_t rows, int64_t ld,
			     size_t *bytes_out, int word = 8, int width = 0)
{
	const int n = width > 0 ? width : c->un;	/* (width: the k words per row of a right-hand side or a solution) */
	if (!ptr && rows != 0)
		return blz_fail(BLZ_EINVAL, "%s: %s is NULL", who, arg);
	if (ld < n)
		return blz_fail(BLZ_EINVAL, "%s: the row stride of %s is %lld words, less than %s = %d", who, arg, (long long)ld,
				width > 0 ? "k" : "n", n);
	if (((uintptr_t)ptr & (uintptr_t)(word - 1)) != 0)
		return blz_fail(BLZ_EINVAL, "%s: %s is not aligned to %d bytes", who, arg, word);
	if (rows < 0 || (word == 8 && (rows > ((int64_t)1 << 40) || ld > ((int64_t)1 << 40))))
		return blz_fail(BLZ_EINVAL, "%s: %s: %lld rows with a row stride of %lld words", who, arg, (long long)rows, (long long)ld);
	if (rows == 0) {
		if (bytes_out)
			*bytes_out = 0;
		return BLZ_OK;
	}
	const unsigned __int128 wide = ((unsigned __int128)(rows - 1) * (unsigned __int128)ld + (unsigned __int128)n) * (unsigned)word;
	if (word == 4 && wide > ((unsigned __int128)1 << 62))
		return blz_fail(BLZ_EINVAL, "%s: %s of %lld rows with a row stride of %lld words leaves 64-bit byte offsets", who, arg,
				(long long)rows, (long long)ld);
	const size_t bytes = (size_t)wide;
	const int rc = devio_check_alloc(c, who, arg, ptr, bytes, rows, ld, width);
	if (rc != BLZ_OK)
		return rc;
	if (bytes_out)
		*bytes_out = bytes;
	return BLZ_OK;
}

/* the same for an operand that is `words` 8-byte words in a row and not a block: d, npiv, info */
static int devio_check_words(const blz_ctx *c, const char *who, const char *arg, const void *ptr, int64_t words, size_t *bytes_out)
{
	if (!ptr)
		return blz_fail(BLZ_EINVAL, "%s: %s is NULL", who, arg);
	if (((uintptr_t)ptr & 7) != 0)
		return blz_fail(BLZ_EINVAL, "%s: %s is not aligned to 8 bytes", who, arg);
	const int rc = devio_check_alloc(c, who, arg, ptr, (size_t)words * 8, 1, words);
	if (rc != BLZ_OK)
		return rc;
	if (bytes_out)
		*bytes_out = (size_t)words * 8;
	return BLZ_OK;
}

static bool devalg_overlap(const void *a, size_t ab, const void *b, size_t bb)
{
	return (const char *)a < (const char *)b + bb && (const char *)b < (const char *)a + ab;
}

/* Ordering on the caller's stream, without the host: our stream waits for everything the caller has enqueued so far
 * (devio_enter), the caller's stream for everything we enqueue (devio_leave).  A capturing stream is refused: the work
 * runs on the context's own streams and cannot become part of the caller's graph. */
static int devio_refuse_capture(const char *who, hipStream_t caller)
{
	hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
	HIPCHK(hipStreamIsCapturing(caller, &cap));
	if (cap != hipStreamCaptureStatusNone)
		return blz_fail(BLZ_EINVAL, "%s: the stream is capturing a graph", who);
	return BLZ_OK;
}

/* What every call on caller-owned blocks asks before it looks at an argument, for blocks of `word`-byte words.  The 32-bit
 * family (word 4) is for a plain single rank and a context of 4-byte words, and says so in its own words. */
static int devio_begin(blz_ctx *c, const char *who, int word, bool need_matrix, void *stream)
{
	if (word == 8) {
		const int rc = devio_refuse_ranks(c, who);
		if (rc != BLZ_OK)
			return rc;
	} else {
		if (!c)
			return blz_fail(BLZ_EINVAL, "%s: NULL context", who);
		if (c->device_ranks)
			return blz_fail(BLZ_EINVAL, "%s: 32-bit device blocks need a plain single rank, and device blocks on ranks are "
					"switched on (blz_set_device_ranks)", who);
		if (c->nranks > 1 || c->comm || c->loop || c->force_comm)
			return blz_fail(BLZ_EINVAL, "%s: 32-bit device blocks need a single rank without a communicator, a loopback group or "
					"BLZ_FORCE_COMM", who);
		if (c->prime >= ((uint64_t)1 << 32) || c->cfg.word != 4)
			return blz_fail(BLZ_EINVAL, "%s: p = %llu: residues do not fit 32-bit words (blz_word_bytes is %d)", who,
					(unsigned long long)c->prime, c->cfg.word);
	}
	if (need_matrix && !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "no matrix loaded (blz_set_matrix)");
	HIPCHK(hipSetDevice(c->device));
	return devio_refuse_capture(who, (hipStream_t)stream);
}

/* the first of the two events: our stream waits for the caller's (no matrix is needed for this much) */
static int devio_wait_caller(blz_ctx *c, hipStream_t caller)
{
	if (!c->ev_caller) {
		HIPCHK(hipEventCreateWithFlags(&c->ev_caller, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&c->ev_ours, hipEventDisableTiming));
	}
	HIPCHK(hipEventRecord(c->ev_caller, caller));
	HIPCHK(hipStreamWaitEvent(c->stream, c->ev_caller, 0));
	return BLZ_OK;
}

static int devio_enter(blz_ctx *c, hipStream_t caller)
{
	if (!c->inv_ready) {	/* once per matrix */
		for (int sd = 0; sd < 2; sd++) {
			if (c->inv[sd].empty())
				continue;
			HIPCHK(hipMalloc((void **)&c->inv_dev[sd], c->inv[sd].size() * sizeof(int32_t)));
			HIPCHK(hipMemcpy(c->inv_dev[sd], c->inv[sd].data(), c->inv[sd].size() * sizeof(int32_t), hipMemcpyHostToDevice));
		}
		c->inv_ready = true;
	}
	return devio_wait_caller(c, caller);
}

static int devio_leave(blz_ctx *c, hipStream_t caller)
{
	HIPCHK(hipEventRecord(c->ev_ours, c->stream));
	HIPCHK(hipStreamWaitEvent(caller, c->ev_ours, 0));
	return BLZ_OK;
}

/* the two scratch slabs of the apply calls, one per side, and control words whose stop flag is never up.  On ranks the rows
 * past count[side] of a slab are never written and stay zero, which the all-gather relies on */
static int devio_apply_scratch(blz_ctx *c)
{
	for (int sd = 0; sd < 2; sd++)
		if (!c->slab[APPLY_SLAB + sd]) {
			const size_t bytes = (size_t)std::max<int64_t>(c->stride[sd], 1) * c->cfg.n * c->cfg.word;
			HIPCHK(hipMalloc(&c->slab[APPLY_SLAB + sd], bytes));
			HIPCHK(hipMemset(c->slab[APPLY_SLAB + sd], 0, bytes));
			c->slab_bytes[APPLY_SLAB + sd] = bytes;
		}
	if (!c->apply_ctl) {
		HIPCHK(hipMalloc((void **)&c->apply_ctl, sizeof(DevCtl)));
		HIPCHK(hipMemset(c->apply_ctl, 0, sizeof(DevCtl)));
	}
	return BLZ_OK;
}

/* slab `slab`, of side sd, <- the caller's block and back, on the context's stream, by the launcher of the caller's word */
template <typename W>
static hipError_t devio_import(blz_ctx *c, int slab, int sd, const W *blk, int64_t ld, unsigned long long *bad)
{
	if constexpr (sizeof(W) == 8)
		return launch_block_import(c->cfg, c->slab[slab], blk, ld, devio_inv(c, sd), c->count[sd], c->un, bad, c->stream);
	else
		return launch_w32_import(c->cfg, c->slab[slab], blk, ld, devio_inv(c, sd), c->count[sd], c->un, bad, c->stream);
}

template <typename W>
static hipError_t devio_export(blz_ctx *c, W *blk, int64_t ld, int slab, int sd)
{
	if constexpr (sizeof(W) == 8)
		return launch_block_export(c->cfg, blk, ld, c->slab[slab], devio_inv(c, sd), c->count[sd], c->un, c->stream);
	else
		return launch_w32_export(c->cfg, blk, ld, c->slab[slab], devio_inv(c, sd), c->count[sd], c->un, c->stream);
}

/* ---- device matrix: M from triplets on the GPU, both CSRs built there (kernels: blz_devmat.hip).
 * A build and a host upload (set_matrix_prepared) differ only in how the slabs are filled.  Both refuse first, then go
 * matrix_begin (the old matrix goes, the geometry and the numbering of the new one are installed), their slabs through
 * alloc_stream_arrays, plan_csr and slab_whole_choices, and matrix_blocks, which alone makes the matrix resident. ---- */

/* device memory of one build: whatever is still listed when the build leaves, by whichever exit, is freed */
struct DevmatTmp {
	std::vector<void *> ptrs;
	~DevmatTmp()
	{
		for (void *p : ptrs)
			hipFree(p);
	}
	hipError_t alloc(void **p, size_t bytes)
	{
		const hipError_t e = hipMalloc(p, bytes ? bytes : 1);
		if (e == hipSuccess)
			ptrs.push_back(*p);
		return e;
	}
	void keep(void *p)	/* it belongs to the context from here on */
	{
		for (auto &q : ptrs)
			if (q == p) {
				q = ptrs.back();
				ptrs.pop_back();
				return;
			}
	}
};

/* BLZ_DEVMAT_TRACE=1: HIP events between the stages of a build or of an ordering.  Each of the two has its own marks and
 * prints its own line on stderr once its stream has been synchronised (tools/device_matrix_cost.py reads both). */
struct StageTrace {
	enum { MAX_MARKS = 8 };
	bool on = false;
	hipStream_t st = nullptr;
	hipEvent_t ev[MAX_MARKS] = {};
	bool set[MAX_MARKS] = {};
	explicit StageTrace(hipStream_t s) : st(s)
	{
		const char *e = getenv("BLZ_DEVMAT_TRACE");
		on = e && e[0] == '1';
	}
	void mark(int k)
	{
		if (on && !set[k] && hipEventCreate(&ev[k]) == hipSuccess) {
			(void)hipEventRecord(ev[k], st);
			set[k] = true;
		}
	}
	bool reached(int k) const { return on && set[k]; }
	float ms(int a, int b)
	{
		float t = 0.0f;
		if (!set[a] || !set[b] || hipEventElapsedTime(&t, ev[a], ev[b]) != hipSuccess)
			return 0.0f;
		return t;
	}
	~StageTrace()
	{
		for (int k = 0; k < MAX_MARKS; k++)
			if (set[k])
				hipEventDestroy(ev[k]);
	}
};

/* everything that is refused before a byte moves: the arguments and the state of the context (pointers: devmat_refuse_ptr) */
static int devmat_refuse(const blz_ctx *c, const char *who, int64_t nrows, int64_t ncols, int64_t nnz, int idx_bytes, const void *x,
			 int val_bytes)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "%s: NULL context", who);
	if (idx_bytes != 4 && idx_bytes != 8)
		return blz_fail(BLZ_EINVAL, "%s: idx_bytes = %d is neither 4 (int32) nor 8 (int64)", who, idx_bytes);
	if (val_bytes != 0 && val_bytes != 4 && val_bytes != 8)
		return blz_fail(BLZ_EINVAL, "%s: val_bytes = %d is not 0 (all ones), 4 (uint32) or 8 (uint64)", who, val_bytes);
	if ((val_bytes == 0 && x) || (val_bytes != 0 && !x && nnz > 0))	/* (no entries: no element is read, any pointer will do) */
		return blz_fail(BLZ_EINVAL, "%s: x and val_bytes disagree (val_bytes = %d with x %s NULL)", who, val_bytes, x ? "not" : "=");
	if (nrows < 0 || ncols < 0 || nrows >= ((int64_t)1 << 31) || ncols >= ((int64_t)1 << 31))
		return blz_fail(BLZ_EINVAL, "%s: nrows = %lld, ncols = %lld: both must lie in [0, 2^31)", who, (long long)nrows, (long long)ncols);
	if (nnz < 0 || nnz >= (int64_t)UINT32_MAX)
		return blz_fail(BLZ_EINVAL, "%s: nnz = %lld must lie in [0, 2^32 - 1)", who, (long long)nnz);
	if (c->values_signed)
		return blz_fail(BLZ_EINVAL, "%s: the context is in signed value mode; the device build takes residues below p", who);
	if (c->wide_hi)
		return blz_fail(BLZ_EINVAL, "%s: high limbs are pending (blz_set_values_wide); the device build takes wide entries as "
				"8-byte values", who);
	if ((c->have_matrix && c->nranks > 1) || c->comm || c->loop || c->force_comm)
		return blz_fail(BLZ_EINVAL, "%s: the device build needs a single rank without a communicator, a loopback group or "
				"BLZ_FORCE_COMM (see DESIGN.md section 22)", who);
	return BLZ_OK;
}

static int devmat_refuse_ptr(const blz_ctx *c, const char *who, const char *arg, const void *ptr, int64_t count, int elem)
{
	if (count == 0)
		return BLZ_OK;		/* no element is read: any pointer will do */
	if (!ptr)
		return blz_fail(BLZ_EINVAL, "%s: %s is NULL", who, arg);
	if (((uintptr_t)ptr & (uintptr_t)(elem - 1)) != 0)
		return blz_fail(BLZ_EINVAL, "%s: %s is not aligned to its %d-byte elements", who, arg, elem);
	return devio_check_alloc(c, who, arg, ptr, (size_t)count * (size_t)elem, count, 1);
}

/* The build itself.  i, j, x have passed devmat_refuse_ptr (or are the library's own copies).  Until the counts of the check
 * pass and the two row_ptr arrays have been read the context is untouched; from there on (matrix_begin) a failure leaves it
 * without a matrix.  perm: NULL for a plain build; an ordered build hands over the numbering i, j are already in, perm[0] of
 * M's rows and perm[1] of its columns (both empty: the identity, the order of a matrix without entries). */
static int devmat_build(blz_ctx *c, const char *who, int64_t nrows, int64_t ncols, int64_t nnz, const void *i, const void *j,
			int idx_bytes, const void *x, int val_bytes, int right, std::vector<int32_t> *perm)
{
	enum { COUNT0 = 0, COUNT1, SCAN1, SCATTER0, SCATTER1, PALETTE1, PACK1 };
	DevmatTmp tmp;
	hipStream_t st = c->stream;
	StageTrace trace(st);
	struct Line {	/* the build's line: by whichever exit, once the build got past the scatter */
		StageTrace &tr;
		~Line()
		{
			if (tr.reached(SCATTER1) && hipStreamSynchronize(tr.st) == hipSuccess)
				fprintf(stderr, "blz device build: check+count %.3f ms, scan %.3f ms, scatter %.3f ms, palette %.3f ms, pack %.3f ms\n",
					tr.ms(COUNT0, COUNT1), tr.ms(COUNT1, SCAN1), tr.ms(SCATTER0, SCATTER1), tr.ms(SCATTER1, PALETTE1),
					tr.ms(PALETTE1, PACK1));
		}
	} line{ trace };
	const int64_t rows_t[2] = { nrows, ncols };	/* rows of CSR(M), of CSR(M^T) */
	u32 *rp[2] = { nullptr, nullptr };
	unsigned long long *counts = nullptr;
	for (int t = 0; t < 2; t++) {
		HIPCHK(tmp.alloc((void **)&rp[t], (size_t)(rows_t[t] + 1) * sizeof(u32)));
		HIPCHK(hipMemsetAsync(rp[t], 0, (size_t)(rows_t[t] + 1) * sizeof(u32), st));
	}
	HIPCHK(tmp.alloc((void **)&counts, DEVMAT_COUNTS * sizeof(unsigned long long)));
	HIPCHK(hipMemsetAsync(counts, 0, DEVMAT_COUNTS * sizeof(unsigned long long), st));
	trace.mark(COUNT0);
	HIPCHK(launch_devmat_count(c->cfg, idx_bytes, val_bytes, i, j, x, nnz, nrows, ncols, rp[0], rp[1], counts, st));
	trace.mark(COUNT1);
	unsigned long long hc[DEVMAT_COUNTS];
	HIPCHK(hipStreamSynchronize(st));
	HIPCHK(hipMemcpy(hc, counts, sizeof hc, hipMemcpyDeviceToHost));
	if (hc[DEVMAT_BAD_ROW] || hc[DEVMAT_BAD_COL] || hc[DEVMAT_BAD_VAL])
		return blz_fail(BLZ_EINVAL, "%s: %llu row indices outside [0, %lld), %llu column indices outside [0, %lld), %llu values "
				"not below p (of %lld entries)", who, hc[DEVMAT_BAD_ROW], (long long)nrows, hc[DEVMAT_BAD_COL],
				(long long)ncols, hc[DEVMAT_BAD_VAL], (long long)nnz);
	u32 *sums = nullptr;
	HIPCHK(tmp.alloc((void **)&sums, (size_t)devmat_scan_tiles(std::max(nrows, ncols) + 1) * sizeof(u32)));
	std::vector<u32> hrp[2];
	for (int t = 0; t < 2; t++) {
		HIPCHK(launch_devmat_scan(rp[t], rows_t[t] + 1, sums, st));
		hrp[t].resize((size_t)rows_t[t] + 1);
	}
	trace.mark(SCAN1);
	HIPCHK(hipStreamSynchronize(st));
	for (int t = 0; t < 2; t++) {
		HIPCHK(hipMemcpy(hrp[t].data(), rp[t], hrp[t].size() * sizeof(u32), hipMemcpyDeviceToHost));
		if (hrp[t][0] != 0 || (int64_t)hrp[t][(size_t)rows_t[t]] != nnz)
			return blz_fail(BLZ_EHIP, "%s: the scan of the %s counts ends at %u, not at nnz = %lld", who, t ? "column" : "row",
					hrp[t][(size_t)rows_t[t]], (long long)nnz);
	}
	/* the choices the host path makes from the values (csr_from_coo_window, upload_csr) */
	const bool pattern = val_bytes == 0 || hc[DEVMAT_NOT_ONE] == 0;
	const bool wide = !pattern && hc[DEVMAT_HIGH] != 0 && c->cfg.word == 8;
	for (int t = 0; t < 2 && wide; t++) {
		const int rcw = wide_refuse_long_row(hrp[t].data(), rows_t[t]);
		if (rcw != BLZ_OK)
			return rcw;
	}

	/* ---- the matrix that was resident goes; the context is that of BLZ_NO_REORDER=1 after blz_set_matrix(M, right, 0, 1),
	 * under the numbering the ordered build hands over ---- */
	MatrixShape S = { right ? 1 : 0, 0, 1, 1, nrows, ncols, { nullptr, nullptr }, { 0, 0 }, {}, { 0.0, 0.0 }, { 1.0, 1.0 }, 0 };
	for (int q = 0; q < 2 && perm; q++)
		S.perm[q] = std::move(perm[q]);
	matrix_begin(c, S);
	c->values_wide = wide;
	u32 *cur[2] = { nullptr, nullptr };
	for (int t = 0; t < 2; t++) {
		DevCsr &D = c->csr[t][0];
		D.rows = rows_t[t];
		D.cols = rows_t[1 - t];
		D.nnz = nnz;
		D.wide = wide;
		D.locality = 1.0;
		D.row_ptr = rp[t];
		tmp.keep(rp[t]);
		/* (the value arrays of a slab that turns out packed go again after the pack) */
		const int rca = alloc_stream_arrays(D, nnz, !pattern, wide, st);
		if (rca != BLZ_OK)
			return rca;
		/* the cursors: a transient copy of the row pointers */
		HIPCHK(tmp.alloc((void **)&cur[t], (size_t)std::max<int64_t>(rows_t[t], 1) * sizeof(u32)));
		HIPCHK(hipMemcpyAsync(cur[t], rp[t], (size_t)rows_t[t] * sizeof(u32), hipMemcpyDeviceToDevice, st));
	}
	{
		DevCsr &A = c->csr[0][0], &B = c->csr[1][0];
		trace.mark(SCATTER0);
		HIPCHK(launch_devmat_scatter(c->cfg, idx_bytes, val_bytes, i, j, x, nnz, nrows, ncols, cur[0], cur[1], A.col_idx, A.val,
					     A.val_hi, B.col_idx, B.val, B.val_hi, st));
		trace.mark(SCATTER1);
	}
	/* Packed stream, by upload_csr's rule: at most 256 distinct values and fewer than 2^24 columns, unless BLZ_NO_PACK.  Both
	 * slabs hold the same values: one palette, made from CSR(M), ascending, serves both. */
	bool packable[2];
	for (int t = 0; t < 2; t++)
		packable[t] = !pattern && c->pack && c->csr[t][0].cols < (1 << 24);
	if (packable[0] || packable[1]) {
		unsigned long long *table = nullptr, *keys = nullptr;
		unsigned int *pcount = nullptr, hcount = 0;
		HIPCHK(tmp.alloc((void **)&table, DEVMAT_PAL_SLOTS * sizeof(unsigned long long)));
		HIPCHK(tmp.alloc((void **)&keys, DEVMAT_PAL_MAX * sizeof(unsigned long long)));
		HIPCHK(tmp.alloc((void **)&pcount, sizeof(unsigned int)));
		HIPCHK(hipMemsetAsync(table, 0xFF, DEVMAT_PAL_SLOTS * sizeof(unsigned long long), st));
		HIPCHK(hipMemsetAsync(pcount, 0, sizeof(unsigned int), st));
		HIPCHK(launch_devmat_palette(c->cfg, c->csr[0][0].val, c->csr[0][0].val_hi, nnz, table, pcount, keys, st));
		trace.mark(PALETTE1);
		HIPCHK(hipStreamSynchronize(st));
		HIPCHK(hipMemcpy(&hcount, pcount, sizeof hcount, hipMemcpyDeviceToHost));
		if (hcount >= 1 && hcount <= DEVMAT_PAL_MAX) {
			std::vector<unsigned long long> hk((size_t)hcount);
			HIPCHK(hipMemcpy(hk.data(), keys, hk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
			std::sort(hk.begin(), hk.end());
			HIPCHK(hipMemcpy(keys, hk.data(), hk.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
			std::vector<u32> pal((size_t)(wide ? 512 : 256), 0u);	/* (wide: 256 low limbs, then 256 high limbs) */
			for (size_t q = 0; q < hk.size(); q++) {
				pal[q] = (u32)hk[q];
				if (wide)
					pal[256 + q] = (u32)(hk[q] >> 32);
			}
			for (int t = 0; t < 2; t++) {
				if (!packable[t])
					continue;
				DevCsr &D = c->csr[t][0];
				HIPCHK(hipMalloc(&D.palette, pal.size() * sizeof(u32)));
				HIPCHK(hipMemcpy(D.palette, pal.data(), pal.size() * sizeof(u32), hipMemcpyHostToDevice));
				HIPCHK(launch_devmat_pack(c->cfg, D.col_idx, D.val, D.val_hi, nnz, keys, (int)hcount, st));
			}
			trace.mark(PACK1);
			HIPCHK(hipStreamSynchronize(st));
			for (int t = 0; t < 2; t++) {
				if (!packable[t])
					continue;
				DevCsr &D = c->csr[t][0];	/* the value arrays of a packed slab were transient */
				hipFree(D.val);
				D.val = nullptr;
				if (D.val_hi)
					hipFree(D.val_hi);
				D.val_hi = nullptr;
			}
		}
	}
	HIPCHK(hipStreamSynchronize(st));
	for (int t = 0; t < 2; t++) {
		const bool dot_slab = carries_dots(c, t);
		const int rc = plan_csr(c, hrp[t].data(), c->csr[t][0], 0, dot_slab);
		if (rc != BLZ_OK)
			return rc;
		slab_whole_choices(c, t, hrp[t].data(), c->csr[t][0].cols, dot_slab, 1, true);
	}
	const int rc = matrix_blocks(c, 1, 1);
	c->device_built = rc == BLZ_OK;
	c->device_order = c->device_built && perm != nullptr;
	return rc;
}

/* The ordered build: blz_reorder's numbering made on the device (csrc/blz_devorder.hip), the triplets
 * relabelled into int32 copies, then devmat_build on those.  Nothing here touches the context: the resident matrix goes only
 * when devmat_build has read the counts of its check pass as zero.  The caller's arrays are only read. */
static int devmat_build_ordered(blz_ctx *c, const char *who, int64_t nrows, int64_t ncols, int64_t nnz, const void *i, const void *j,
				int idx_bytes, const void *x, int val_bytes, int right)
{
	std::vector<int32_t> num[2];	/* the new index of every row, of every column */
	if (nnz == 0)		/* nothing to order by: the identity, as blz_prepare leaves a matrix without entries */
		return devmat_build(c, who, nrows, ncols, nnz, i, j, idx_bytes, x, val_bytes, right, num);
	enum { BEGIN = 0, MIN0, SORT0, MIN1, SORT1, RELABEL };
	DevmatTmp tmp;
	hipStream_t st = c->stream;
	StageTrace trace(st);
	const int64_t longer = std::max(nrows, ncols), dims[2] = { nrows, ncols };
	int32_t *key = nullptr, *perm[2] = { nullptr, nullptr }, *bkey[2], *bitem[2], *ni = nullptr, *nj = nullptr;
	u32 *counters = nullptr, *sums = nullptr;
	HIPCHK(tmp.alloc((void **)&key, (size_t)longer * sizeof(int32_t)));
	for (int q = 0; q < 2; q++) {
		HIPCHK(tmp.alloc((void **)&perm[q], (size_t)dims[q] * sizeof(int32_t)));
		HIPCHK(tmp.alloc((void **)&bkey[q], (size_t)longer * sizeof(int32_t)));
		HIPCHK(tmp.alloc((void **)&bitem[q], (size_t)longer * sizeof(int32_t)));
	}
	HIPCHK(tmp.alloc((void **)&counters, (size_t)devorder_sort_counters(longer) * sizeof(u32)));
	HIPCHK(tmp.alloc((void **)&sums, (size_t)devmat_scan_tiles(devorder_sort_counters(longer)) * sizeof(u32)));
	HIPCHK(tmp.alloc((void **)&ni, (size_t)nnz * sizeof(int32_t)));
	HIPCHK(tmp.alloc((void **)&nj, (size_t)nnz * sizeof(int32_t)));
	trace.mark(BEGIN);
	/* rows by smallest column (rows without entries: ncols, last), then columns by smallest NEW row */
	for (int q = 0; q < 2; q++) {
		HIPCHK(launch_devorder_fill(c->cfg, key, dims[q], (int32_t)dims[1 - q], st));
		HIPCHK(launch_devorder_min(c->cfg, idx_bytes, i, j, nnz, nrows, ncols, q ? perm[0] : nullptr, key, q, st));
		trace.mark(q ? MIN1 : MIN0);
		HIPCHK(launch_devorder_sort(c->cfg, key, dims[q], dims[1 - q], perm[q], bkey, bitem, counters, sums, st));
		trace.mark(q ? SORT1 : SORT0);
	}
	HIPCHK(launch_devorder_relabel(c->cfg, idx_bytes, i, j, nnz, nrows, ncols, perm[0], perm[1], ni, nj, st));
	trace.mark(RELABEL);
	HIPCHK(hipStreamSynchronize(st));
	if (trace.reached(RELABEL))
		fprintf(stderr, "blz device order: row keys %.3f ms, row sort %.3f ms, column keys %.3f ms, column sort %.3f ms, "
			"relabel %.3f ms\n", trace.ms(BEGIN, MIN0), trace.ms(MIN0, SORT0), trace.ms(SORT0, MIN1), trace.ms(MIN1, SORT1),
			trace.ms(SORT1, RELABEL));
	/* the numbering on the host, once: the host blocks, the right-hand sides and the checkpoints go through it */
	for (int q = 0; q < 2; q++) {
		num[q].resize((size_t)dims[q]);
		if (dims[q] > 0)
			HIPCHK(hipMemcpy(num[q].data(), perm[q], (size_t)dims[q] * sizeof(int32_t), hipMemcpyDeviceToHost));
		std::vector<bool> taken((size_t)dims[q], false);
		for (int64_t r = 0; r < dims[q]; r++) {
			const int64_t to = num[q][(size_t)r];
			if (to < 0 || to >= dims[q] || taken[(size_t)to])
				return blz_fail(BLZ_EHIP, "%s: the device sort of the %s did not return a permutation (at %lld)", who,
						q ? "columns" : "rows", (long long)r);
			taken[(size_t)to] = true;
		}
	}
	/* the transients of the sort go before the build allocates the two CSRs */
	for (void *p : { (void *)key, (void *)perm[0], (void *)perm[1], (void *)bkey[0], (void *)bkey[1], (void *)bitem[0],
			 (void *)bitem[1], (void *)counters, (void *)sums }) {
		tmp.keep(p);
		hipFree(p);
	}
	return devmat_build(c, who, nrows, ncols, nnz, ni, nj, 4, x, val_bytes, right, num);
}

static int devmat_refuse_order(const char *who, int order)
{
	if (order != 0 && order != 1)
		return blz_fail(BLZ_EINVAL, "%s: order = %d is neither 0 (the caller's numbering) nor 1 (rows by smallest column, columns "
				"by smallest new row)", who, order);
	return BLZ_OK;
}

static int devmat_set_device(blz_ctx *c, const char *who, int64_t nrows, int64_t ncols, int64_t nnz, const void *i, const void *j,
			     int idx_bytes, const void *x, int val_bytes, int right, int order, void *stream)
{
	int rc = devmat_refuse(c, who, nrows, ncols, nnz, idx_bytes, x, val_bytes);
	if (rc != BLZ_OK)
		return rc;
	if ((rc = devmat_refuse_order(who, order)) != BLZ_OK)
		return rc;
	if ((rc = devio_refuse_capture(who, (hipStream_t)stream)) != BLZ_OK)
		return rc;
	HIPCHK(hipSetDevice(c->device));
	if ((rc = devmat_refuse_ptr(c, who, "i", i, nnz, idx_bytes)) != BLZ_OK ||
	    (rc = devmat_refuse_ptr(c, who, "j", j, nnz, idx_bytes)) != BLZ_OK ||
	    (val_bytes && (rc = devmat_refuse_ptr(c, who, "x", x, nnz, val_bytes)) != BLZ_OK))
		return rc;
	if ((rc = devio_wait_caller(c, (hipStream_t)stream)) != BLZ_OK)
		return rc;
	if (order)
		return devmat_build_ordered(c, who, nrows, ncols, nnz, i, j, idx_bytes, x, val_bytes, right);
	return devmat_build(c, who, nrows, ncols, nnz, i, j, idx_bytes, x, val_bytes, right, nullptr);
}

extern "C" int blz_set_matrix_device(blz_ctx *c, int64_t nrows, int64_t ncols, int64_t nnz, const void *i, const void *j,
				     int idx_bytes, const void *x, int val_bytes, int right, void *stream)
{
	return devmat_set_device(c, "blz_set_matrix_device", nrows, ncols, nnz, i, j, idx_bytes, x, val_bytes, right, 0, stream);
}

extern "C" int blz_set_matrix_device_ordered(blz_ctx *c, int64_t nrows, int64_t ncols, int64_t nnz, const void *i, const void *j,
					     int idx_bytes, const void *x, int val_bytes, int right, int order, void *stream)
{
	return devmat_set_device(c, "blz_set_matrix_device_ordered", nrows, ncols, nnz, i, j, idx_bytes, x, val_bytes, right, order,
				 stream);
}

static int devmat_set_upload(blz_ctx *c, const char *who, const blz_coo *M, int right, int order)
{
	if (!c || !M)
		return blz_fail(BLZ_EINVAL, "%s: NULL argument", who);
	if (M->nnz >= (int64_t)UINT32_MAX)
		return blz_fail(BLZ_EINVAL, "%s: nnz >= 2^32 per slab is not supported", who);
	if (M->nnz > 0 && (!M->i || !M->j || !M->x))
		return blz_fail(BLZ_EINVAL, "%s: the triplets of M are NULL", who);
	int rc = devmat_refuse(c, who, M->nrows, M->ncols, M->nnz, 4, M->x, 4);
	if (rc != BLZ_OK)
		return rc;
	if ((rc = devmat_refuse_order(who, order)) != BLZ_OK)
		return rc;
	HIPCHK(hipSetDevice(c->device));
	DevmatTmp tmp;		/* the triplets on the device, for the length of the call */
	void *dev[3] = { nullptr, nullptr, nullptr };
	const void *host[3] = { M->i, M->j, M->x };
	const size_t bytes = (size_t)M->nnz * 4;
	for (int q = 0; q < 3; q++) {
		HIPCHK(tmp.alloc(&dev[q], bytes));
		if (bytes)
			HIPCHK(hipMemcpy(dev[q], host[q], bytes, hipMemcpyHostToDevice));
	}
	if (order)
		return devmat_build_ordered(c, who, M->nrows, M->ncols, M->nnz, dev[0], dev[1], 4, dev[2], 4, right);
	return devmat_build(c, who, M->nrows, M->ncols, M->nnz, dev[0], dev[1], 4, dev[2], 4, right, nullptr);
}

extern "C" int blz_set_matrix_upload(blz_ctx *c, const blz_coo *M, int right)
{
	return devmat_set_upload(c, "blz_set_matrix_upload", M, right, 0);
}

extern "C" int blz_set_matrix_upload_ordered(blz_ctx *c, const blz_coo *M, int right, int order)
{
	return devmat_set_upload(c, "blz_set_matrix_upload_ordered", M, right, order);
}

extern "C" int blz_matrix_device_built(const blz_ctx *c) { return c && c->have_matrix && c->device_built ? 1 : 0; }

extern "C" int blz_matrix_device_order(const blz_ctx *c)
{
	return c && c->have_matrix && c->device_built && c->device_order ? 1 : 0;
}

extern "C" int blz_numbering(const blz_ctx *c, int block, int32_t *perm)
{
	if (!c || !perm || block < 0 || block > 3)
		return blz_fail(BLZ_EINVAL, "blz_numbering: no context, no array or block %d", block);
	if (c->have_matrix && c->nranks > 1)
		return blz_fail(BLZ_EINVAL, "blz_numbering: the context holds one rank of %d", c->nranks);
	const int sd = side_of(block);
	const int64_t rows = c->glob_rows[sd];
	if (!c->have_matrix || c->perm[sd].empty()) {
		for (int64_t r = 0; r < rows; r++)
			perm[r] = (int32_t)r;
		return 0;
	}
	memcpy(perm, c->perm[sd].data(), (size_t)rows * sizeof(int32_t));
	return 1;
}

/* The calls below are written once for both word widths of a caller's block: W is uint64_t for blz_..._device and uint32_t
 * for blz_..._device32, `who` the name the caller used.  The widths differ in what devio_begin refuses,
 * in the word size of devio_check_range and in the launcher of the last line. */

template <typename W>
static int devio_set_block(blz_ctx *c, const char *who, int block, const W *dev, int64_t ld, void *stream, int64_t *bad)
{
	int rc = devio_begin(c, who, sizeof(W), true, stream);
	if (rc != BLZ_OK)
		return rc;
	if (block < 0 || block > 3)
		return blz_fail(BLZ_EINVAL, "%s: block %d is not one of V, TMP, AV, P", who, block);
	const int sd = side_of(block);
	if ((rc = devio_check_range(c, who, "dev", dev, devio_rows(c, sd), ld, nullptr, sizeof(W))) != BLZ_OK)
		return rc;
	if (bad && !c->bad_dev)
		HIPCHK(hipMalloc((void **)&c->bad_dev, sizeof(unsigned long long)));
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_enter(c, caller)) != BLZ_OK)
		return rc;
	if (block == BLZ_P) {	/* p is what the caller says from here on (explicit_p_state, on the stream) */
		HIPCHK(launch_identity_tail(c->small, c->cfg.n, c->stream));
		c->p_implicit = false;
	}
	if (bad)
		HIPCHK(hipMemsetAsync(c->bad_dev, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(devio_import(c, block, sd, dev, ld, bad ? c->bad_dev : nullptr));
	if (c->gath_holds[sd] == block)
		c->gath_holds[sd] = -1;		/* on ranks: the gathered copy is of the rows the block had before */
	if ((rc = devio_leave(c, caller)) != BLZ_OK)
		return rc;
	if (bad) {
		unsigned long long cnt = 0;
		HIPCHK(hipStreamSynchronize(c->stream));
		HIPCHK(hipMemcpy(&cnt, c->bad_dev, sizeof cnt, hipMemcpyDeviceToHost));
		*bad = (int64_t)cnt;
		if (cnt)
			return blz_fail(BLZ_EINVAL, "%s: %llu words of the block are not residues below p", who, cnt);
	}
	return BLZ_OK;
}

extern "C" int blz_set_block_device(blz_ctx *c, int block, const uint64_t *dev, int64_t ld, void *stream, int64_t *bad)
{
	return devio_set_block(c, "blz_set_block_device", block, dev, ld, stream, bad);
}

template <typename W>
static int devio_get_block(blz_ctx *c, const char *who, int block, W *dev, int64_t ld, void *stream)
{
	int rc = devio_begin(c, who, sizeof(W), true, stream);
	if (rc != BLZ_OK)
		return rc;
	if (block < 0 || block > 3)
		return blz_fail(BLZ_EINVAL, "%s: block %d is not one of V, TMP, AV, P", who, block);
	const int sd = side_of(block);
	if ((rc = devio_check_range(c, who, "dev", dev, devio_rows(c, sd), ld, nullptr, sizeof(W))) != BLZ_OK)
		return rc;
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_enter(c, caller)) != BLZ_OK)
		return rc;
	if (block == BLZ_P && c->p_implicit) {	/* materialize_p, on the stream */
		const int np = c->cfg.n;
		HIPCHK(launch_block_mul(c->cfg, c->slab[BLZ_P], c->count[0], np, np, c->small + small_E(np), c->stream));
		HIPCHK(launch_identity_tail(c->small, np, c->stream));
		c->p_implicit = false;
	}
	HIPCHK(devio_export(c, dev, ld, block, sd));
	return devio_leave(c, caller);
}

extern "C" int blz_get_block_device(blz_ctx *c, int block, uint64_t *dev, int64_t ld, void *stream)
{
	return devio_get_block(c, "blz_get_block_device", block, dev, ld, stream);
}

extern "C" int blz_apply_rows(const blz_ctx *c, int transpose, int64_t *x_rows, int64_t *y_rows)
{
	if (!c || !c->have_matrix)
		return blz_fail(BLZ_EINVAL, "no matrix loaded (blz_set_matrix)");
	const int ys = c->row_side[transpose ? 1 : 0];
	if (x_rows)
		*x_rows = devio_rows(c, 1 - ys);
	if (y_rows)
		*y_rows = devio_rows(c, ys);
	return BLZ_OK;
}

template <typename W>
static int devio_apply(blz_ctx *c, const char *who, int transpose, const W *x, int64_t ldx, W *y, int64_t ldy, void *stream)
{
	int rc = devio_begin(c, who, sizeof(W), true, stream);
	if (rc != BLZ_OK)
		return rc;
	const int t = transpose ? 1 : 0, ys = c->row_side[t], xs = 1 - ys;
	size_t xb = 0, yb = 0;
	if ((rc = devio_check_range(c, who, "x", x, devio_rows(c, xs), ldx, &xb, sizeof(W))) != BLZ_OK ||
	    (rc = devio_check_range(c, who, "y", y, devio_rows(c, ys), ldy, &yb, sizeof(W))) != BLZ_OK)
		return rc;
	if (devalg_overlap(x, xb, y, yb))
		return blz_fail(BLZ_EINVAL, "%s: x and y overlap", who);
	if ((rc = devrank_refuse_product(c, who, t)) != BLZ_OK)
		return rc;
	/* (on ranks the product is collective from here on: an error exit tells the loopback peers) */
	auto enqueue = [&]() -> int {
		int rc_ = devio_apply_scratch(c);
		if (rc_ != BLZ_OK)
			return rc_;
		hipStream_t caller = (hipStream_t)stream;
		if ((rc_ = devio_enter(c, caller)) != BLZ_OK)
			return rc_;
		HIPCHK(devio_import(c, APPLY_SLAB + xs, xs, x, ldx, nullptr));
		if ((rc_ = enqueue_product(c, t, APPLY_SLAB + xs, APPLY_SLAB + ys, false, nullptr, c->apply_ctl)) != BLZ_OK)
			return rc_;
		HIPCHK(devio_export(c, y, ldy, APPLY_SLAB + ys, ys));
		return devio_leave(c, caller);
	};
	return devrank_collective_exit(c, enqueue());
}

extern "C" int blz_apply_device(blz_ctx *c, int transpose, const uint64_t *x, int64_t ldx, uint64_t *y, int64_t ldy, void *stream)
{
	return devio_apply(c, "blz_apply_device", transpose, x, ldx, y, ldy, stream);
}

extern "C" int blz_apply_release(blz_ctx *c)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "blz_apply_release: NULL context");
	HIPCHK(hipSetDevice(c->device));
	if (c->stream)
		HIPCHK(hipStreamSynchronize(c->stream));
	for (int sd = 0; sd < 2; sd++) {
		if (c->slab[APPLY_SLAB + sd])
			HIPCHK(hipFree(c->slab[APPLY_SLAB + sd]));
		c->slab[APPLY_SLAB + sd] = nullptr;
		c->slab_bytes[APPLY_SLAB + sd] = 0;
	}
	if (c->apply_ctl)
		HIPCHK(hipFree(c->apply_ctl));
	c->apply_ctl = nullptr;
	return BLZ_OK;
}

/* ---- device block algebra: X^T * Y and sum_t X_t * A_t on caller-owned device memory (kernels: blz_devalg.hip; DESIGN.md
 * section 16).  No matrix is needed and nothing of a solve is read or written: the only state is the scratch of the dot. ---- */

/* The ONE decision whether a 64-bit call takes the matrix-core form (blz_devmfma_plan.h): the launch
 * sites below and blz_devalg_plan ask here.  aligned16: every tall block's base is 16-byte aligned and every ld even. */
static int devmfma_decide(const blz_ctx *c, int op, int64_t rows, int nterms, bool aligned16, dm_plan *pl)
{
	dm_env e;
	e.mfma = c->cfg.mfma;
	e.word_bytes = c->cfg.word;
	e.p_is_m61 = c->cfg.mers == 61;
	e.n = c->un;
	e.num_cu = c->cfg.num_cu;
	memcpy(e.min_rows, c->devmfma_min_rows, sizeof e.min_rows);
	return dm_decide(&e, op, rows, nterms, aligned16 ? 1 : 0, pl);
}

static bool devmfma_aligned(const void *b, int64_t ld)
{
	return ((uintptr_t)b & 15) == 0 && (ld & 1) == 0;
}

extern "C" int blz_devalg_plan(const blz_ctx *c, int op, int64_t rows, int nterms, int aligned16, struct blz_devalg_plan *out)
{
	if (!c || !out)
		return blz_fail(BLZ_EINVAL, "blz_devalg_plan: no context or out is NULL");
	if (op != BLZ_DEVOP_DOT && op != BLZ_DEVOP_DOT_PAIR && op != BLZ_DEVOP_COMBINE && op != BLZ_DEVOP_COMBINE_PAIR)
		return blz_fail(BLZ_EINVAL, "blz_devalg_plan: op = %d is none of BLZ_DEVOP_DOT, BLZ_DEVOP_DOT_PAIR, BLZ_DEVOP_COMBINE, "
				"BLZ_DEVOP_COMBINE_PAIR", op);
	if (nterms < 1 || nterms > BLZ_MAX_TERMS)
		return blz_fail(BLZ_EINVAL, "blz_devalg_plan: nterms = %d is outside 1..%d", nterms, BLZ_MAX_TERMS);
	dm_plan pl;
	if (devmfma_decide(c, op, rows, nterms, aligned16 != 0, &pl) != 0)
		return blz_fail(BLZ_EINVAL, "blz_devalg_plan: op = %d, nterms = %d", op, nterms);
	memset(out, 0, sizeof *out);
	out->form = pl.form;
	out->min_rows = pl.min_rows;
	out->tile_rows = pl.tile_rows;
	out->wavefronts = pl.wavefronts;
	out->fold_tiles = pl.fold_tiles;
	out->lds_bytes = pl.lds_bytes;
	return BLZ_OK;
}

/* the inner products of both arities and both word widths: nx = 1 writes n * n words, nx = 2 two contiguous panels (the fused
 * call of DESIGN.md section 18, in its own kernel and with a scratch of its own) */
template <typename W>
static int devalg_dot(blz_ctx *c, const char *who, int64_t rows, int nx, const W *const *x, const int64_t *ldx, const W *y,
		      int64_t ldy, uint64_t *out, void *stream)
{
	int rc = devio_begin(c, who, sizeof(W), false, stream);
	if (rc != BLZ_OK)
		return rc;
	if (rows < 0)
		return blz_fail(BLZ_EINVAL, "%s: rows = %lld is negative", who, (long long)rows);
	const int n = c->un;
	static const char *const xname[2][2] = { { "x", "" }, { "x0", "x1" } };
	size_t xb[2] = { 0, 0 }, yb = 0, cb = 0;
	long long ldl[2] = { 0, 0 };
	for (int k = 0; k < nx; k++) {
		if ((rc = devio_check_range(c, who, xname[nx - 1][k], x[k], rows, ldx[k], &xb[k], sizeof(W))) != BLZ_OK)
			return rc;
		ldl[k] = ldx[k];
	}
	if ((rc = devio_check_range(c, who, "y", y, rows, ldy, &yb, sizeof(W))) != BLZ_OK ||
	    (rc = devio_check_words(c, who, "c", out, (int64_t)nx * n * n, &cb)) != BLZ_OK)
		return rc;
	for (int k = 0; k < nx; k++)
		if (devalg_overlap(out, cb, x[k], xb[k]))
			return blz_fail(BLZ_EINVAL, "%s: c overlaps %s", who, xname[nx - 1][k]);
	if (devalg_overlap(out, cb, y, yb))
		return blz_fail(BLZ_EINVAL, "%s: c overlaps y", who);
	int N = 1;
	bool collective = false;	/* (never, for 32-bit words: they are not on ranks) */
	if ((rc = devrank_dot_ranks(c, who, &N, &collective)) != BLZ_OK)
		return rc;
	auto enqueue = [&]() -> int {
		u64 **partial = nx == 1 ? &c->devalg_partial : &c->devfuse_partial;
		if (!*partial)
			HIPCHK(hipMalloc((void **)partial, (size_t)dev_dot_max_blocks(c->cfg, n) * nx * n * n * sizeof(u64)));
		int rc_ = collective ? devrank_dot_buffers(c) : BLZ_OK;
		if (rc_ != BLZ_OK)
			return rc_;
		hipStream_t caller = (hipStream_t)stream;
		if ((rc_ = devio_wait_caller(c, caller)) != BLZ_OK)
			return rc_;
		/* on ranks: this rank's residues into the send buffer, their sums over the ranks (both panels through one all-reduce),
		 * the sums' residues into c */
		u64 *dst = collective ? c->devrank_send : out;
		if constexpr (sizeof(W) == 4) {
			HIPCHK(launch_w32_dot(c->cfg, n, rows, nx, x, ldl, y, ldy, *partial, dst, c->stream));
		} else {
			dm_plan pl;
			bool al = devmfma_aligned(y, ldy);
			for (int k = 0; k < nx; k++)
				al = al && devmfma_aligned(x[k], ldx[k]);
			if (devmfma_decide(c, nx == 1 ? DM_OP_DOT : DM_OP_DOT_PAIR, rows, 1, al, &pl) != 0)
				return blz_fail(BLZ_EINVAL,"%s: no plan", who);
			if (pl.form == 1)	/* (the scratch of either arity holds at least dev_dot_max_blocks() of its rows) */
				HIPCHK(launch_devmfma_dot(pl, n, rows, nx, x[0], ldl[0], nx == 2 ? x[1] : nullptr, ldl[nx - 1], y, ldy,
							  *partial, dev_dot_max_blocks(c->cfg, n), dst, c->stream));
			else
				HIPCHK(launch_dev_dot(c->cfg, n, rows, nx, x, ldl, y, ldy, *partial, dst, c->stream));
		}
		if (collective && (rc_ = devrank_dot_finish(c, out, nx * n * n)) != BLZ_OK)
			return rc_;
		return devio_leave(c, caller);
	};
	return collective ? devrank_collective_exit(c, enqueue()) : enqueue();
}

extern "C" int blz_dot_device(blz_ctx *c, int64_t rows, const uint64_t *x, int64_t ldx, const uint64_t *y, int64_t ldy,
			      uint64_t *out, void *stream)
{
	return devalg_dot<uint64_t>(c, "blz_dot_device", rows, 1, &x, &ldx, y, ldy, out, stream);
}

/* the recombinations of both arities and both word widths: nz = 1 has a0 and z0 only, nz = 2 is the fused call */
template <typename W>
static int devalg_combine(blz_ctx *c, const char *who, int64_t rows, int nterms, const W *const *x, const int64_t *ldx, int nz,
			  const uint64_t *const *a0, const uint64_t *const *a1, W *z0, int64_t ldz0, W *z1, int64_t ldz1, void *stream)
{
	int rc = devio_begin(c, who, sizeof(W), false, stream);
	if (rc != BLZ_OK)
		return rc;
	if (nterms < 1 || nterms > BLZ_MAX_TERMS)
		return blz_fail(BLZ_EINVAL, "%s: nterms = %d is outside 1..%d", who, nterms, BLZ_MAX_TERMS);
	if (rows < 0)
		return blz_fail(BLZ_EINVAL, "%s: rows = %lld is negative", who, (long long)rows);
	if (!x || !ldx || !a0 || (nz == 2 && !a1))
		return blz_fail(BLZ_EINVAL, "%s: the array of %s is NULL", who, !x ? "x" : !ldx ? "ldx" : !a0 ? (nz == 2 ? "a0" : "a") : "a1");
	const uint64_t *const *a[2] = { a0, a1 };
	W *z[2] = { z0, z1 };
	const int64_t ldz[2] = { ldz0, ldz1 };
	if (nz == 2) {
		int in[2] = { 0, 0 };
		for (int t = 0; t < nterms; t++) {
			if (!a0[t] && !a1[t])
				return blz_fail(BLZ_EINVAL, "%s: term %d enters neither output (a0[%d] and a1[%d] are both NULL)", who, t, t, t);
			in[0] += a0[t] != nullptr;
			in[1] += a1[t] != nullptr;
		}
		for (int o = 0; o < 2; o++)
			if (!in[o])
				return blz_fail(BLZ_EINVAL, "%s: output z%d has no term (every a%d[t] is NULL)", who, o, o);
	}
	const int n = c->un;
	size_t xb[BLZ_MAX_TERMS] = { 0 }, ab[2][BLZ_MAX_TERMS] = { { 0 } }, zb[2] = { 0, 0 };
	long long ldl[BLZ_MAX_TERMS] = { 0 };
	char nm[12], zn[2][4] = { "z", "" };
	if (nz == 2)
		for (int o = 0; o < 2; o++)
			snprintf(zn[o], sizeof zn[o], "z%d", o);
	for (int t = 0; t < nterms; t++) {
		snprintf(nm, sizeof nm, "x[%d]", t);
		if ((rc = devio_check_range(c, who, nm, x[t], rows, ldx[t], &xb[t], sizeof(W))) != BLZ_OK)
			return rc;
		for (int o = 0; o < nz; o++) {
			if (nz == 2)
				snprintf(nm, sizeof nm, "a%d[%d]", o, t);
			else
				snprintf(nm, sizeof nm, "a[%d]", t);
			/* (a coefficient of the pair may be NULL: the term does not enter that output) */
			if ((nz == 1 || a[o][t]) && (rc = devio_check_range(c, who, nm, a[o][t], n, n, &ab[o][t])) != BLZ_OK)
				return rc;
		}
		ldl[t] = ldx[t];
	}
	for (int o = 0; o < nz; o++)
		if ((rc = devio_check_range(c, who, zn[o], z[o], rows, ldz[o], &zb[o], sizeof(W))) != BLZ_OK)
			return rc;
	if (nz == 2 && rows > 0 && devalg_overlap(z0, zb[0], z1, zb[1]))
		return blz_fail(BLZ_EINVAL, "%s: z0 overlaps z1", who);
	for (int o = 0; o < nz; o++)
		for (int t = 0; t < nterms; t++) {
			const bool in_place = x[t] == z[o] && ldx[t] == ldz[o];
			if (!in_place && devalg_overlap(z[o], zb[o], x[t], xb[t]))
				return blz_fail(BLZ_EINVAL, "%s: %s overlaps x[%d] without being it (the in-place form is the same pointer "
						"and the same stride)", who, zn[o], t);
			for (int q = 0; q < nz; q++) {
				if (!a[q][t] || !devalg_overlap(z[o], zb[o], a[q][t], ab[q][t]))
					continue;
				if (nz == 2)
					return blz_fail(BLZ_EINVAL, "%s: z%d overlaps a%d[%d]", who, o, q, t);
				return blz_fail(BLZ_EINVAL, "%s: z overlaps a[%d]", who, t);
			}
		}
	if (rows == 0)
		return BLZ_OK;	/* the outputs have no words */
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_wait_caller(c, caller)) != BLZ_OK)
		return rc;
	if constexpr (sizeof(W) == 4) {
		HIPCHK(launch_w32_combine(c->cfg, n, rows, nterms, x, ldl, nz, a0, a1, z0, ldz0, z1, ldz1, c->stream));
	} else {
		dm_plan pl;
		bool al = true;
		for (int o = 0; o < nz; o++)
			al = al && devmfma_aligned(z[o], ldz[o]);
		for (int t = 0; t < nterms; t++)
			al = al && devmfma_aligned(x[t], ldx[t]);
		if (devmfma_decide(c, nz == 1 ? DM_OP_COMBINE : DM_OP_COMBINE_PAIR, rows, nterms, al, &pl) != 0)
			return blz_fail(BLZ_EINVAL,"%s: no plan", who);
		if (pl.form == 1) {
			if (!c->devmfma_img)
				HIPCHK(hipMalloc((void **)&c->devmfma_img, (size_t)dm_image_bytes_max()));
			HIPCHK(launch_devmfma_combine(pl, n, rows, nterms, x, ldl, a0, nz == 2 ? a1 : nullptr, z0, ldz0, z1, ldz1,
						      c->devmfma_img, c->stream));
		} else {
			HIPCHK(launch_dev_combine(c->cfg, n, rows, nterms, x, ldl, nz, a0, a1, z0, ldz0, z1, ldz1, c->stream));
		}
	}
	return devio_leave(c, caller);
}

extern "C" int blz_combine_device(blz_ctx *c, int64_t rows, int nterms, const uint64_t *const *x, const int64_t *ldx,
				  const uint64_t *const *a, uint64_t *z, int64_t ldz, void *stream)
{
	return devalg_combine<uint64_t>(c, "blz_combine_device", rows, nterms, x, ldx, 1, a, nullptr, z, ldz, nullptr, 0, stream);
}

/* ---- fused device calls: z = op2 (op1 x), two inner products against one block, two recombinations of shared inputs, each in
 * one call and one pass (kernels: blz_devalg.hip).  Nothing of a solve is read or written: the state is
 * the scratch slabs and control words of blz_apply_device and a scratch of blz_dot_pair_device's own. ---- */

template <typename W>
static int devfuse_apply_pair(blz_ctx *c, const char *who, int transpose_first, const W *x, int64_t ldx, W *y, int64_t ldy, W *z,
			      int64_t ldz, void *stream)
{
	int rc = devio_begin(c, who, sizeof(W), true, stream);
	if (rc != BLZ_OK)
		return rc;
	const int t = transpose_first ? 1 : 0, ys = c->row_side[t], xs = 1 - ys;
	size_t xb = 0, yb = 0, zb = 0;
	if ((rc = devio_check_range(c, who, "x", x, devio_rows(c, xs), ldx, &xb, sizeof(W))) != BLZ_OK ||
	    (y && (rc = devio_check_range(c, who, "y", y, devio_rows(c, ys), ldy, &yb, sizeof(W))) != BLZ_OK) ||
	    (rc = devio_check_range(c, who, "z", z, devio_rows(c, xs), ldz, &zb, sizeof(W))) != BLZ_OK)
		return rc;
	const bool in_place = (const W *)z == x && ldz == ldx;
	if (!in_place && devalg_overlap(z, zb, x, xb))
		return blz_fail(BLZ_EINVAL, "%s: z overlaps x without being it (the in-place form is the same pointer and the same "
				"stride)", who);
	if (y && devalg_overlap(y, yb, x, xb))
		return blz_fail(BLZ_EINVAL, "%s: y overlaps x", who);
	if (y && devalg_overlap(y, yb, z, zb))
		return blz_fail(BLZ_EINVAL, "%s: y overlaps z", who);
	if ((rc = devrank_refuse_product(c, who, t)) != BLZ_OK || (rc = devrank_refuse_product(c, who, 1 - t)) != BLZ_OK)
		return rc;
	auto enqueue = [&]() -> int {	/* (collective on ranks, as the single product) */
		int rc_ = devio_apply_scratch(c);
		if (rc_ != BLZ_OK)
			return rc_;
		hipStream_t caller = (hipStream_t)stream;
		if ((rc_ = devio_enter(c, caller)) != BLZ_OK)
			return rc_;
		HIPCHK(devio_import(c, APPLY_SLAB + xs, xs, x, ldx, nullptr));
		if ((rc_ = enqueue_product(c, t, APPLY_SLAB + xs, APPLY_SLAB + ys, false, nullptr, c->apply_ctl)) != BLZ_OK)
			return rc_;
		if (y)	/* the intermediate is wanted: one pass more; otherwise it lives in its slab only */
			HIPCHK(devio_export(c, y, ldy, APPLY_SLAB + ys, ys));
		/* back into the slab x was imported to: the first product has consumed it (so z may be x) */
		if ((rc_ = enqueue_product(c, 1 - t, APPLY_SLAB + ys, APPLY_SLAB + xs, false, nullptr, c->apply_ctl)) != BLZ_OK)
			return rc_;
		HIPCHK(devio_export(c, z, ldz, APPLY_SLAB + xs, xs));
		return devio_leave(c, caller);
	};
	return devrank_collective_exit(c, enqueue());
}

extern "C" int blz_apply_pair_device(blz_ctx *c, int transpose_first, const uint64_t *x, int64_t ldx, uint64_t *y, int64_t ldy,
				     uint64_t *z, int64_t ldz, void *stream)
{
	return devfuse_apply_pair(c, "blz_apply_pair_device", transpose_first, x, ldx, y, ldy, z, ldz, stream);
}

extern "C" int blz_dot_pair_device(blz_ctx *c, int64_t rows, const uint64_t *x0, int64_t ldx0, const uint64_t *x1, int64_t ldx1,
				   const uint64_t *y, int64_t ldy, uint64_t *out, void *stream)
{
	const uint64_t *x[2] = { x0, x1 };
	const int64_t ldx[2] = { ldx0, ldx1 };
	return devalg_dot<uint64_t>(c, "blz_dot_pair_device", rows, 2, x, ldx, y, ldy, out, stream);
}

extern "C" int blz_combine_pair_device(blz_ctx *c, int64_t rows, int nterms, const uint64_t *const *x, const int64_t *ldx,
				       const uint64_t *const *a0, const uint64_t *const *a1, uint64_t *z0, int64_t ldz0, uint64_t *z1,
				       int64_t ldz1, void *stream)
{
	return devalg_combine(c, "blz_combine_pair_device", rows, nterms, x, ldx, 2, a0, a1, z0, ldz0, z1, ldz1, stream);
}

/* ---- device small algebra: the n x n chain of a Krylov step and the echelon form of a caller's block (kernels:
 * blz_devsmall.hip).  No matrix is needed and nothing of a solve is read or written: the only state is
 * the stack and the control words of blz_rref_device, which are this call's own. ---- */

struct DevRange {
	const char *name;
	const void *ptr;
	size_t bytes;
};

/* no output may overlap an input or another output: outs[0 .. nout) against each other and against ins[0 .. nin) */
static int devsmall_refuse_overlap(const char *who, const DevRange *outs, int nout, const DevRange *ins, int nin)
{
	for (int a = 0; a < nout; a++) {
		if (!outs[a].ptr)
			continue;
		for (int b = 0; b < nin; b++)
			if (ins[b].bytes && devalg_overlap(outs[a].ptr, outs[a].bytes, ins[b].ptr, ins[b].bytes))
				return blz_fail(BLZ_EINVAL, "%s: %s overlaps %s", who, outs[a].name, ins[b].name);
		for (int b = a + 1; b < nout; b++)
			if (outs[b].ptr && devalg_overlap(outs[a].ptr, outs[a].bytes, outs[b].ptr, outs[b].bytes))
				return blz_fail(BLZ_EINVAL, "%s: %s overlaps %s", who, outs[a].name, outs[b].name);
	}
	return BLZ_OK;
}

static int devsmall_begin(blz_ctx *c, const char *who, void *stream)
{
	int rc = devio_refuse_ranks(c, who);
	if (rc != BLZ_OK)
		return rc;
	HIPCHK(hipSetDevice(c->device));
	return devio_refuse_capture(who, (hipStream_t)stream);
}

extern "C" int blz_semi_inverse_device(blz_ctx *c, const uint64_t *vtav, uint64_t *winv, uint64_t *d, uint64_t *npiv, void *stream)
{
	static const char who[] = "blz_semi_inverse_device";
	int rc = devsmall_begin(c, who, stream);
	if (rc != BLZ_OK)
		return rc;
	const int n = c->un;
	DevRange in = { "vtav", vtav, 0 }, out[3] = { { "winv", winv, 0 }, { "d", d, 0 }, { "npiv", npiv, 0 } };
	if ((rc = devio_check_range(c, who, "vtav", vtav, n, n, &in.bytes)) != BLZ_OK ||
	    (rc = devio_check_range(c, who, "winv", winv, n, n, &out[0].bytes)) != BLZ_OK ||
	    (rc = devio_check_words(c, who, "d", d, n, &out[1].bytes)) != BLZ_OK ||
	    (npiv && (rc = devio_check_words(c, who, "npiv", npiv, 1, &out[2].bytes)) != BLZ_OK))
		return rc;
	if ((rc = devsmall_refuse_overlap(who, out, 3, &in, 1)) != BLZ_OK)
		return rc;
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_wait_caller(c, caller)) != BLZ_OK)
		return rc;
	HIPCHK(launch_dev_chain(c->cfg, n, vtav, nullptr, winv, d, nullptr, npiv, c->stream));
	return devio_leave(c, caller);
}

extern "C" int blz_ortho_coeffs_device(blz_ctx *c, const uint64_t *vtav, const uint64_t *vtaav, uint64_t *coef, uint64_t *npiv,
				       void *stream)
{
	static const char who[] = "blz_ortho_coeffs_device";
	int rc = devsmall_begin(c, who, stream);
	if (rc != BLZ_OK)
		return rc;
	const int n = c->un;
	DevRange in[2] = { { "vtav", vtav, 0 }, { "vtaav", vtaav, 0 } }, out[2] = { { "coef", coef, 0 }, { "npiv", npiv, 0 } };
	if ((rc = devio_check_range(c, who, "vtav", vtav, n, n, &in[0].bytes)) != BLZ_OK ||
	    (rc = devio_check_range(c, who, "vtaav", vtaav, n, n, &in[1].bytes)) != BLZ_OK ||
	    (rc = devio_check_words(c, who, "coef", coef, (int64_t)BLZ_COEF_PANELS * n * n, &out[0].bytes)) != BLZ_OK ||
	    (npiv && (rc = devio_check_words(c, who, "npiv", npiv, 1, &out[1].bytes)) != BLZ_OK))
		return rc;
	if ((rc = devsmall_refuse_overlap(who, out, 2, in, 2)) != BLZ_OK)
		return rc;
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_wait_caller(c, caller)) != BLZ_OK)
		return rc;
	HIPCHK(launch_dev_chain(c->cfg, n, vtav, vtaav, nullptr, nullptr, coef, npiv, c->stream));
	return devio_leave(c, caller);
}

extern "C" int blz_rref_device(blz_ctx *c, int64_t rows, const uint64_t *x, int64_t ldx, uint64_t *e, uint64_t *z, int64_t *info,
			       void *stream)
{
	static const char who[] = "blz_rref_device";
	int rc = devsmall_begin(c, who, stream);
	if (rc != BLZ_OK)
		return rc;
	if (c->device_ranks && (c->nranks > 1 || c->comm || c->loop || c->force_comm))
		return blz_fail(BLZ_EINVAL, "%s: the echelon on ranks is not built (the row space of a block spread over ranks needs a "
				"merge of the ranks' echelons); the call needs a plain single rank (DESIGN.md section 20)", who);
	if (rows < 0)
		return blz_fail(BLZ_EINVAL, "%s: rows = %lld is negative", who, (long long)rows);
	const int n = c->un;
	DevRange in = { "x", x, 0 }, out[3] = { { "e", e, 0 }, { "z", z, 0 }, { "info", info, 0 } };
	/* the kernel indexes a row as row * ldx in 64 signed bits (devio_check_range admits 2^40 of either) */
	if (rows > 0 && ldx >= n && ldx > (INT64_MAX / 8) / rows)
		return blz_fail(BLZ_EINVAL, "%s: %lld rows at a row stride of ldx = %lld words are beyond 64-bit byte offsets", who,
				(long long)rows, (long long)ldx);
	if ((rc = devio_check_range(c, who, "x", x, rows, ldx, &in.bytes)) != BLZ_OK)
		return rc;
	if ((rc = devio_check_range(c, who, "e", e, n, n, &out[0].bytes)) != BLZ_OK ||
	    (z && (rc = devio_check_range(c, who, "z", z, n, n, &out[1].bytes)) != BLZ_OK) ||
	    (rc = devio_check_words(c, who, "info", info, (int64_t)n + 1, &out[2].bytes)) != BLZ_OK)
		return rc;
	if ((rc = devsmall_refuse_overlap(who, out, 3, &in, 1)) != BLZ_OK)
		return rc;
	if (!c->devsmall_stack)
		HIPCHK(hipMalloc((void **)&c->devsmall_stack, (size_t)dev_rref_stack_rows(c->cfg, n) * n * sizeof(u64)));
	if (!c->devsmall_ctl)
		HIPCHK(hipMalloc((void **)&c->devsmall_ctl, 2 * sizeof(int)));
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_wait_caller(c, caller)) != BLZ_OK)
		return rc;
	HIPCHK(launch_dev_rref(c->cfg, n, rows, x, ldx, c->devsmall_stack, c->devsmall_ctl, e, z, (long long *)info, c->stream));
	return devio_leave(c, caller);
}

/* ---- the bridges of device blocks on ranks: a whole block (blz_rows x n, the file's numbering) and the rank's own rows of it
 * (blz_local_rows x n, slab order).  Row-local copies on the context's stream; nothing of a solve is read or written. ---- */

static int devrank_bridge(blz_ctx *c, const char *who, int block, const uint64_t *whole, int64_t ldw, const uint64_t *local,
			  int64_t ldl, void *stream, bool take)
{
	if (!c)
		return blz_fail(BLZ_EINVAL, "%s: NULL context", who);
	if (!c->device_ranks)
		return blz_fail(BLZ_EINVAL, "%s: device blocks on ranks are not switched on (blz_set_device_ranks)", who);
	int rc = devio_refuse_ranks(c, who);
	if (rc != BLZ_OK)
		return rc;
	NEED_MATRIX(c);
	if ((rc = devio_refuse_capture(who, (hipStream_t)stream)) != BLZ_OK)
		return rc;
	if (block < 0 || block > 3)
		return blz_fail(BLZ_EINVAL, "%s: block %d is not one of V, TMP, AV, P", who, block);
	const int sd = side_of(block);
	size_t wb = 0, lb = 0;
	if ((rc = devio_check_range(c, who, "global", whole, c->glob_rows[sd], ldw, &wb)) != BLZ_OK ||
	    (rc = devio_check_range(c, who, "local", local, c->count[sd], ldl, &lb)) != BLZ_OK)
		return rc;
	if (wb && lb && devalg_overlap(whole, wb, local, lb))
		return blz_fail(BLZ_EINVAL, "%s: local overlaps global", who);
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_enter(c, caller)) != BLZ_OK)
		return rc;
	if (take)
		HIPCHK(launch_rows_take(c->cfg, const_cast<uint64_t *>(local), ldl, whole, ldw, c->inv_dev[sd], c->first[sd], c->count[sd],
					c->un, c->stream));
	else
		HIPCHK(launch_rows_put(c->cfg, const_cast<uint64_t *>(whole), ldw, local, ldl, c->inv_dev[sd], c->first[sd], c->count[sd],
				       c->un, c->stream));
	return devio_leave(c, caller);
}

extern "C" int blz_take_local_device(blz_ctx *c, int block, const uint64_t *global, int64_t ldg, uint64_t *local, int64_t ldl,
				     void *stream)
{
	return devrank_bridge(c, "blz_take_local_device", block, global, ldg, local, ldl, stream, true);
}

extern "C" int blz_put_local_device(blz_ctx *c, int block, const uint64_t *local, int64_t ldl, uint64_t *global, int64_t ldg,
				    void *stream)
{
	return devrank_bridge(c, "blz_put_local_device", block, global, ldg, local, ldl, stream, false);
}

/* ---- 32-bit device blocks: the family above on a caller's blocks of uint32_t words, for contexts of 4-byte words (p < 2^32;
 * kernels: blz_devw32.hip).  Each call writes the words its 64-bit namesake writes, truncated; the n x n
 * operands stay u64, the scratch is the namesake's (the apply slabs, devalg_partial, devfuse_partial), and the two families
 * interleave freely on one context.  A plain single rank only: no device blocks on ranks, no echelon.  The bodies are the
 * namesakes', at W = uint32_t. ---- */

extern "C" int blz_set_block_device32(blz_ctx *c, int block, const uint32_t *dev, int64_t ld, void *stream, int64_t *bad)
{
	return devio_set_block(c, "blz_set_block_device32", block, dev, ld, stream, bad);
}

extern "C" int blz_get_block_device32(blz_ctx *c, int block, uint32_t *dev, int64_t ld, void *stream)
{
	return devio_get_block(c, "blz_get_block_device32", block, dev, ld, stream);
}

extern "C" int blz_apply_device32(blz_ctx *c, int transpose, const uint32_t *x, int64_t ldx, uint32_t *y, int64_t ldy, void *stream)
{
	return devio_apply(c, "blz_apply_device32", transpose, x, ldx, y, ldy, stream);
}

extern "C" int blz_apply_pair_device32(blz_ctx *c, int transpose_first, const uint32_t *x, int64_t ldx, uint32_t *y, int64_t ldy,
				       uint32_t *z, int64_t ldz, void *stream)
{
	return devfuse_apply_pair(c, "blz_apply_pair_device32", transpose_first, x, ldx, y, ldy, z, ldz, stream);
}

extern "C" int blz_dot_device32(blz_ctx *c, int64_t rows, const uint32_t *x, int64_t ldx, const uint32_t *y, int64_t ldy,
				uint64_t *out, void *stream)
{
	return devalg_dot<uint32_t>(c, "blz_dot_device32", rows, 1, &x, &ldx, y, ldy, out, stream);
}

extern "C" int blz_dot_pair_device32(blz_ctx *c, int64_t rows, const uint32_t *x0, int64_t ldx0, const uint32_t *x1, int64_t ldx1,
				     const uint32_t *y, int64_t ldy, uint64_t *out, void *stream)
{
	const uint32_t *x[2] = { x0, x1 };
	const int64_t ldx[2] = { ldx0, ldx1 };
	return devalg_dot<uint32_t>(c, "blz_dot_pair_device32", rows, 2, x, ldx, y, ldy, out, stream);
}

extern "C" int blz_combine_device32(blz_ctx *c, int64_t rows, int nterms, const uint32_t *const *x, const int64_t *ldx,
				    const uint64_t *const *a, uint32_t *z, int64_t ldz, void *stream)
{
	return devalg_combine<uint32_t>(c, "blz_combine_device32", rows, nterms, x, ldx, 1, a, nullptr, z, ldz, nullptr, 0, stream);
}

extern "C" int blz_combine_pair_device32(blz_ctx *c, int64_t rows, int nterms, const uint32_t *const *x, const int64_t *ldx,
					 const uint64_t *const *a0, const uint64_t *const *a1, uint32_t *z0, int64_t ldz0, uint32_t *z1,
					 int64_t ldz1, void *stream)
{
	return devalg_combine(c, "blz_combine_pair_device32", rows, nterms, x, ldx, 2, a0, a1, z0, ldz0, z1, ldz1, stream);
}

/* ---- device right-hand sides: b from device memory into the border, the solution from the slab into device memory (kernels:
 * blz_devrhs.hip).  A plain single rank only.  Written once for both word widths of the caller's block,
 * like the device blocks above. ---- */

/* what both calls refuse before they look at an argument: the family's refusals, and device blocks on ranks (which the 64-bit
 * device blocks welcome: the border of this path is not distributed) */
static int devrhs_begin(blz_ctx *c, const char *who, int word, void *stream)
{
	if (c && c->device_ranks)
		return blz_fail(BLZ_EINVAL, "%s: a device right-hand side needs a plain single rank, and device blocks on ranks are "
				"switched on (blz_set_device_ranks)", who);
	return devio_begin(c, who, word, true, stream);
}

template <typename W>
static int devrhs_set(blz_ctx *c, const char *who, int k, const W *b, int64_t ldb, void *stream)
{
	int rc = devrhs_begin(c, who, sizeof(W), stream);
	if (rc != BLZ_OK || (rc = rhs_block_refuse_k(c, who, k)) != BLZ_OK)
		return rc;
	if ((rc = rhs_refuse_pieces(c, who, k)) != BLZ_OK)
		return rc;
	const int64_t len = c->glob_rows[1];
	if ((rc = devio_check_range(c, who, "b", b, len, ldb, nullptr, sizeof(W), k)) != BLZ_OK)
		return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	const int kw = border_row_words(k);
	std::vector<int64_t> rows, own;
	char why[512] = "";
	if ((rc = border_locate(c, who, k, k == 1, rows, own, why, sizeof why)) != BLZ_OK)
		return rc;
	if (why[0])
		return blz_fail(BLZ_EINVAL, "%s", why);
	/* the import goes into a fresh buffer, zero filled like the host's: the border that is resident applies until the count
	 * has been read as zero */
	DevmatTmp tmp;
	void *fresh = nullptr;
	const size_t fresh_bytes = (size_t)std::max<int64_t>(len, 1) * kw * c->cfg.word;
	HIPCHK(tmp.alloc(&fresh, fresh_bytes));
	if (!c->bad_dev)
		HIPCHK(hipMalloc((void **)&c->bad_dev, sizeof(unsigned long long)));
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_enter(c, caller)) != BLZ_OK)
		return rc;
	unsigned long long cnt = 0;
	{
		/* (from the first enqueue on nothing returns before the stream has drained: `fresh` is freed on the way out) */
		hipError_t e = hipMemsetAsync(c->bad_dev, 0, sizeof(unsigned long long), c->stream);
		if (e == hipSuccess && len == 0)
			e = hipMemsetAsync(fresh, 0, fresh_bytes, c->stream);
		if (e == hipSuccess)
			e = launch_rhs_import<W>(c->cfg, fresh, b, ldb, c->inv_dev[1], len, k, kw, c->bad_dev, c->stream);
		rc = e == hipSuccess ? devio_leave(c, caller) : BLZ_OK;
		const hipError_t e2 = hipStreamSynchronize(c->stream);
		HIPCHK(e);
		HIPCHK(e2);
		if (rc != BLZ_OK)
			return rc;
		HIPCHK(hipMemcpy(&cnt, c->bad_dev, sizeof cnt, hipMemcpyDeviceToHost));
	}
	if (cnt)
		return blz_fail(BLZ_EINVAL, "%s: %llu words of b are not below p", who, cnt);
	tmp.keep(fresh);	/* (border_install's from here on) */
	return border_install(c, k, rows, nullptr, fresh);
}

extern "C" int blz_set_rhs_device(blz_ctx *c, int k, const uint64_t *b, int64_t ldb, void *stream)
{
	return devrhs_set(c, "blz_set_rhs_device", k, b, ldb, stream);
}

extern "C" int blz_set_rhs_device32(blz_ctx *c, int k, const uint32_t *b, int64_t ldb, void *stream)
{
	return devrhs_set(c, "blz_set_rhs_device32", k, b, ldb, stream);
}

template <typename W>
static int devrhs_solution(blz_ctx *c, const char *who, W *x, int64_t ldx, int *status, void *stream)
{
	int rc = devrhs_begin(c, who, sizeof(W), stream);
	if (rc != BLZ_OK)
		return rc;
	if (!c->bd.rhs)
		return blz_fail(BLZ_EINVAL, "%s: the context has no right-hand side (blz_set_rhs_device)", who);
	if (!status)
		return blz_fail(BLZ_EINVAL, "%s: status is NULL", who);
	const int k = c->bd.k;
	const int64_t xrows = c->glob_rows[0] - k;
	if ((rc = devio_check_range(c, who, "x", x, xrows, ldx, nullptr, sizeof(W), k)) != BLZ_OK)
		return rc;
	hipStream_t caller = (hipStream_t)stream;
	if ((rc = devio_enter(c, caller)) != BLZ_OK)
		return rc;
	/* (from here on the caller's stream is ordered behind whatever has been enqueued, on an error exit too) */
	bool verified = false;
	rc = solution_block_reduce(c, status, &verified);
	hipError_t e = hipSuccess;
	if (rc == BLZ_OK && verified)	/* (a failed verification leaves x untouched: nothing is launched) */
		e = launch_solution_export<W>(c->cfg, x, ldx, c->slab[BLZ_V], c->inv_dev[0], c->count[0], xrows, k, c->stream);
	const int rc_leave = devio_leave(c, caller);
	if (rc != BLZ_OK)
		return rc;	/* (the message of the first failure may have been replaced by devio_leave's, the code is the first's) */
	HIPCHK(e);
	return rc_leave;
}

extern "C" int blz_solution_device(blz_ctx *c, uint64_t *x, int64_t ldx, int *status, void *stream)
{
	return devrhs_solution(c, "blz_solution_device", x, ldx, status, stream);
}

extern "C" int blz_solution_device32(blz_ctx *c, uint32_t *x, int64_t ldx, int *status, void *stream)
{
	return devrhs_solution(c, "blz_solution_device32", x, ldx, status, stream);
}

