// On-chip conjugate gradients, the host side: the one launch of k_cg_persist (persist_kernel.h) over the instantiations of
// persist_shapes.h, and the auxiliary kernels around it -- the streaming kernels' inbox exchange, the edge blocks, the node
// marks.  This object holds the main row list; persist_inst.hip holds the others.
#include <cstring>

#include <hip/hip_runtime.h>

#include "persist_kernel.h"
#include "persist_shapes.h"

namespace magk {

// ========================================= inbox exchange for the STREAMING kernels ===
// Meshes the chips cannot hold (more than ~0.5M nodes per GPU: BASELINE config 5 on 8 GPUs) run one fused launch per CG
// iteration, and the ranks must trade [dot partials | q on the interface nodes] between launches.  One RCCL all-reduce
// does that in 20-30 us; this kernel does it through the same per-rank inboxes the on-chip kernel uses (device memory,
// mapped by the peers; tagged granules, polls in local HBM), in place on the buffer the iteration kernel just filled --
// a drop-in for the all-reduce, the iteration kernels are untouched:
//   * q of an interface node this rank owns goes to the inboxes of the ranks that read it (reader mask);
//   * block 0 adds the rank's G partial slots in a fixed order and stores the rank's four sums into every inbox;
//   * block 0 waits for the R sums, adds them in rank order (the same bits on every rank) and writes the total into slot 0
//     of each partial array, clearing the other slots: the next launch's sum over the slots is the total; every block
//     waits for the q of its share of the interface nodes this rank reads and writes them into the buffer; slots the
//     rank neither owns nor reads get 0.
// Epochs alternate between two parities of the inbox; nobody can be two exchanges ahead of a rank that has not finished
// reading (it would need that rank's next sums first).  Every wait is bounded: a rank that gives up raises
// FusedState::exchange_timeout (and the other ranks' timeout words) and the host falls back to the all-reduce.
struct StreamExchangeParams {
    double *buf;              // [4 x g_all partial slots | n_iface x double2 q]: the iteration kernel's output, in place
    int32_t g_all, n_iface, rank, nranks, own0, own1, fpar; // fpar: parity of the iteration launch that filled buf
    uint32_t spin_limit;
    const int32_t *iface;     // sorted Hilbert ids of the interface nodes
    const uint8_t *iface_readers;
    uint8_t *inbox[8];
    FusedState *st;
};

__global__ void __launch_bounds__(256) k_stream_exchange(const StreamExchangeParams P)
{
    __shared__ double s_red[4][4];
    __shared__ double2 s_recs[16];
    const int tid = threadIdx.x, R = P.nranks;
    if (P.st->done) return; // converged (or capped) earlier in this block: every rank takes the same exit
    // Exchange e follows iteration launch e - 1, which left its successor's number e in jslot[fpar ^ 1] (fused_step): the
    // epoch, the inbox parity and the tag come from device memory, identical on every rank (all ranks run the same
    // launches), and nothing in this kernel's arguments changes from one iteration to the next.
    const uint32_t epoch = (uint32_t)P.st->jslot[P.fpar ^ 1];
    const int32_t xpar = (int32_t)(epoch & 1u);
    const uint32_t xtag = P.st->exchange_tag_base + epoch;
    uint8_t *mine = P.inbox[P.rank];
    gu32 *wtmo = (gu32 *)mine;
    double2 *q = (double2 *)(P.buf + 4 * (size_t)P.g_all);
    const size_t qoff = 64 + 128 * (size_t)R;
    // (1) this rank's interface q to their readers
    for (int32_t k = blockIdx.x * 256 + tid; k < P.n_iface; k += gridDim.x * 256) {
        const int32_t g = P.iface[k];
        if (g < P.own0 || g >= P.own1) continue;
        uint32_t readers = P.iface_readers[k];
        double2 v = q[k];
        // both landed before the first store: a load still in flight at the loop's entry would put a wait for the memory
        // counter -- which also counts the stores -- at the top of every round: one store round trip across xGMI per reader
        asm volatile("" : "+v"(readers), "+v"(v.x), "+v"(v.y));
        for (int r = 0; r < R; ++r)
            if (r != P.rank && ((readers >> r) & 1u))
                put_granules_sys((unsigned long long *)(P.inbox[r] + qoff + 32 * ((size_t)xpar * P.n_iface + k)), xtag, v);
    }
    // (2) block 0: the rank's sums, fixed order (thread-strided partials, wave trees, the four waves in order)
    if (blockIdx.x == 0) {
        double S[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < P.g_all; i += 256) {
#pragma unroll
            for (int c = 0; c < 4; ++c) S[c] += P.buf[(size_t)c * P.g_all + i];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) S[c] = wave_sum_dpp(S[c]);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) s_red[c][tid >> 6] = S[c];
        }
        __syncthreads();
        if (tid < 2 * R) {
            double T[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) T[c] = ((s_red[c][0] + s_red[c][1]) + s_red[c][2]) + s_red[c][3];
            put_granules_sys((unsigned long long *)(P.inbox[tid >> 1] + 64) + 4 * (2 * ((int64_t)xpar * R + P.rank) + (tid & 1)),
                             xtag, (tid & 1) == 0 ? make_double2(T[0], T[1]) : make_double2(T[2], T[3]));
        }
    }
    // (3) wait: the R sums (every block) and the q this rank reads (each block its share of the slots)
    const unsigned long long *wrec = (const unsigned long long *)(mine + 64) + 8 * (int64_t)xpar * R;
    const unsigned long long *wq = (const unsigned long long *)(mine + qoff) + 4 * (int64_t)xpar * P.n_iface;
    bool have_w = tid >= 2 * R || blockIdx.x != 0; // only block 0 turns the sums into the next launch's input
    int32_t k = blockIdx.x * 256 + tid; // one slot at a time per thread
    bool ok_all = false;
    for (unsigned spins = 0; spins < P.spin_limit; ++spins) {
        if (!have_w) {
            double2 v;
            have_w = get_granules_sys(wrec, 64u * (uint32_t)R, 32u * (uint32_t)tid, xtag, v);
            if (have_w) s_recs[tid] = v;
        }
        while (k < P.n_iface) { // advance over the slots that are settled; stop at the first one still on its way
            const int32_t g = P.iface[k];
            const bool owned = g >= P.own0 && g < P.own1;
            if (!owned) {
                if ((P.iface_readers[k] >> P.rank) & 1u) {
                    double2 v;
                    if (!get_granules_sys(wq, 32u * (uint32_t)P.n_iface, 32u * (uint32_t)k, xtag, v)) break;
                    q[k] = v;
                } else {
                    q[k] = make_double2(0.0, 0.0);
                }
            }
            k += gridDim.x * 256;
        }
        if (__syncthreads_and((have_w && k >= P.n_iface) ? 1 : 0)) {
            ok_all = true;
            break;
        }
        if ((spins & 255u) == 255u) {
            const int dead = tid == 0 && __hip_atomic_load(wtmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u ? 1 : 0;
            if (__syncthreads_or(dead)) break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    if (!ok_all) {
        if (tid == 0) { // the solve is over for this rank: every later launch of the block exits at once, the host sees
            P.st->exchange_timeout = 1; // `done`, finds the flag and lets the ranks agree on the all-reduce path
            P.st->done = 1;
        }
        if (tid < R) __hip_atomic_store((gu32 *)P.inbox[tid], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    // (4) block 0: totals in rank order into slot 0, the other slots cleared
    if (blockIdx.x == 0) {
        if (tid < 4) {
            const double *rec = (const double *)s_recs;
            double t = 0.0;
            for (int r = 0; r < R; ++r) t += rec[4 * r + tid];
            P.buf[(size_t)tid * P.g_all] = t;
        }
        for (int i = 1 + tid; i < P.g_all; i += 256) {
#pragma unroll
            for (int c = 0; c < 4; ++c) P.buf[(size_t)c * P.g_all + i] = 0.0;
        }
    }
}

void stream_exchange_launch(double *buf, int32_t g_all, int32_t n_iface, int32_t rank, int32_t nranks, int32_t own0,
                            int32_t own1, int32_t fpar, uint32_t spin_limit, const int32_t *iface,
                            const uint8_t *iface_readers, void *const *inboxes, FusedState *st, hipStream_t s)
{
    StreamExchangeParams P = {};
    P.buf = buf;
    P.g_all = g_all;
    P.n_iface = n_iface;
    P.rank = rank;
    P.nranks = nranks;
    P.own0 = own0;
    P.own1 = own1;
    P.fpar = fpar;
    P.spin_limit = spin_limit;
    P.iface = iface;
    P.iface_readers = iface_readers;
    for (int r = 0; r < nranks && r < 8; ++r) P.inbox[r] = (uint8_t *)inboxes[r];
    P.st = st;
    int blocks = (n_iface + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 32 ? 32 : blocks);
    k_stream_exchange<<<blocks, 256, 0, s>>>(P);
}

int persist_tiles_per_wg(int32_t B)
{
    return B == 256 || B == 512 ? kPersistNpt * kPersistThreads / B : 0;
}

// dynamic LDS of a launch; every instantiation also carries 256 bytes of static LDS (the library's __syncthreads_and / _or),
// which the host's fit test adds (kPersistStaticLds)
size_t persist_lds_bytes(int32_t B, int32_t cap, int32_t maxh, int eb_mode, int32_t pool, bool mg)
{
    const size_t tiles = (size_t)persist_tiles_per_wg(B);
    const size_t capx = eb_mode == 2 ? (size_t)B : (size_t)cap; // with overflow blocks the first area holds q of the owned nodes only
    return tiles * (capx + (size_t)cap + (size_t)maxh + (size_t)B) * 16 + 2 * 256 * 16 +
           (4 * (size_t)(kPersistThreads / 64) + 4 + 4 * 32 + kPersistPartDoubles) * 8 + 16 + (eb_mode == 2 ? 32 * (size_t)pool : 0) +
           (mg ? 4 * (size_t)(kPersistNpt * kPersistThreads) : 0); // several ranks: the interface words (s_opk)
}

// The stamped build (no -DMAG_PERSIST_SPLIT_K4) keeps the k4 row in this unit; the product takes it from persist_k4.o.
#ifndef MAG_PERSIST_SPLIT_K4
#define MAG_PERSIST_SPLIT_K4 0
#endif
PersistKernel persist_kernel_K4(const PersistShape &sh);
PersistKernel persist_kernel_CASES(const PersistShape &sh);
PersistKernel persist_kernel_VARIANTS(const PersistShape &sh);
static PersistKernel persist_kernel_MAIN(const PersistShape &sh)
{
#define MAG_PERSIST_ROW(...) MAG_PERSIST_ROW_KERNEL(PERSIST_SINGLE, __VA_ARGS__)
    MAG_PERSIST_ROWS_MAIN(MAG_PERSIST_ROW)
#if MAG_PERSIST_SPLIT_K4
    return persist_kernel_K4(sh);
#else
    MAG_PERSIST_ROWS_K4(MAG_PERSIST_ROW)
    return nullptr;
#endif
#undef MAG_PERSIST_ROW
}

// Every launch of the on-chip kernel: the shape (persist_shapes.h), the kernel from the object that holds it, `members` problems
// side by side (grid.y; PERSIST_SINGLE: 1).  false: no instantiation for this shape, nothing launched.
bool persist_launch(const PersistParams &P, int32_t B, int32_t grid, int32_t members, PersistMembers m, int eb_mode, hipStream_t s)
{
    PersistShape sh;
    if (members < 1 || !persist_shape(B, P.nranks, grid, P.tiles_per_wg, eb_mode, m, sh)) return false;
    const PersistKernel k = m == PERSIST_CASES      ? persist_kernel_CASES(sh)
                            : m == PERSIST_VARIANTS ? persist_kernel_VARIANTS(sh)
                                                    : persist_kernel_MAIN(sh);
    if (!k) return false;
    const size_t lds = persist_lds_bytes(B, P.cap, P.maxh, eb_mode, P.pool_cap, sh.mg);
    k<<<dim3((unsigned)grid, (unsigned)members), 512, lds, s>>>(P);
    return true;
}

int persist_block_entries() { return kPersistBlockEntries; }

// The edge blocks of every node (cg_device.h, ring_blocks), once per solve: one thread per node of the padded Hilbert order
// reads its ring words (tile-local ids) and the coordinates of its neighbours from the tile tables in memory -- owned nodes
// from xyP, halo nodes from the tile's contiguous halo copy -- and writes the 3 NB numbers, value-major (the on-chip kernel's
// loads are coalesced).  Only launched for meshes k_ring16 found to qualify (every row one fan of at most NB entries, or
// NB + 1 closing onto the first).
// VAR: the blocks of variant blockIdx.y, from its coordinates and material constants into its extent of P.kblocks
template <int B, bool VAR = false>
__global__ void __launch_bounds__(256) k_edge_blocks(const PersistParams Pk, double *kbg_)
{
    PersistParams Pv; // (VAR only)
    if constexpr (VAR) Pv = persist_variant_operator(Pk);
    const PersistParams &P = VAR ? Pv : Pk;
    double *kbg = VAR ? const_cast<double *>(P.kblocks) : kbg_;
    constexpr int NB = kPersistBlockEntries, NW = (NB + 2) / 2;
    // (several ranks: the blocks of this rank's own tiles only -- the launcher's grid covers [t0, t1))
    const int64_t nd = (P.nranks > 1 ? (int64_t)P.t0 * B : 0) + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t t = (int32_t)(nd / B), lt = (int32_t)(nd % B);
    if (t >= (P.nranks > 1 ? P.t1 : P.T)) return;
    const TileMeta tm = P.meta[t];
    double kb[3 * NB];
#pragma unroll
    for (int c = 0; c < 3 * NB; ++c) kb[c] = 0.0;
    if (nd < P.N && tm.ent > 0) {
        uint32_t w[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = k < tm.deg ? P.ell16[tm.ell_off + lt + (int64_t)k * B] : 0xffffffffu;
        auto xy_of = [&](uint32_t lid) -> double2 {
            if (lid < (uint32_t)B) {
                const int64_t g = (int64_t)t * B + lid;
                return g < P.N ? P.xyP[g] : make_double2(0.0, 0.0);
            }
            return P.halo_xy[tm.hoff + (int32_t)(lid - B)];
        };
        ring_blocks<NW, NB, 0xfffu>(w, tm.ent < 2 * NW ? tm.ent : 2 * NW, xy_of, P.xyP[nd], P.c0, P.nu, P.h, kb);
    }
#pragma unroll
    for (int c = 0; c < 3 * NB; ++c) kbg[(int64_t)c * P.kb_stride + nd] = kb[c];
}

// The same for meshes whose rows are single fans of ANY length (EBM == 2).  The row is streamed from the ring table, one
// triangle at a time: triangle k (between entries k - 1 and k) contributes its K_ab to block k - 1 and its K_ac to block k --
// or to block 0 when it closes the fan (the row's last entry repeats its first: row_info bit 6), so a closed fan of valence
// v is v blocks.  Block j >= 1 is complete once triangle j + 1 is through; block 0 is held to the end.  Blocks below NB go to
// the value-major arrays the registers are loaded from, block j >= NB to the node's overflow records, at ovf_off[node] +
// j - NB, with the ring entry (tile-local id) it multiplies.  Per block the same two-term sums in the same order as
// ring_blocks: a structured mesh gets the same bits from either kernel.
template <int B, bool VAR = false>
__global__ void __launch_bounds__(256) k_edge_blocks_ovf(const PersistParams Pk, double *kbg_)
{
    PersistParams Pv; // (VAR only)
    if constexpr (VAR) Pv = persist_variant_operator(Pk);
    const PersistParams &P = VAR ? Pv : Pk;
    double *kbg = VAR ? const_cast<double *>(P.kblocks) : kbg_;
    constexpr int NB = kPersistBlockEntries;
    const int64_t nd = (P.nranks > 1 ? (int64_t)P.t0 * B : 0) + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t t = (int32_t)(nd / B), lt = (int32_t)(nd % B);
    if (t >= (P.nranks > 1 ? P.t1 : P.T)) return;
    const TileMeta tm = P.meta[t];
    const uint32_t info = nd < P.N ? P.row_info[nd] : 0u;
    const int32_t n = (info & 0x80u) ? (int32_t)(info & 63u) : 0;
    const bool closed = (info & 0x40u) != 0;
    const int32_t nblk = closed ? n - 1 : n;
    auto emit = [&](int32_t j, double v0, double v1, double v2, uint32_t id) {
        if (j < NB) {
            kbg[(int64_t)(3 * j + 0) * P.kb_stride + nd] = v0;
            kbg[(int64_t)(3 * j + 1) * P.kb_stride + nd] = v1;
            kbg[(int64_t)(3 * j + 2) * P.kb_stride + nd] = v2;
        } else {
            double2 *rec = (double2 *)P.ovf_rec + 2 * ((int64_t)P.ovf_off[nd] + (j - NB));
            rec[0] = make_double2(v0, v1);
            rec[1] = make_double2(v2, __hiloint2double(0, (int)id));
        }
    };
    for (int32_t j = nblk > 0 ? nblk : 0; j < NB; ++j) emit(j, 0.0, 0.0, 0.0, 0u); // blocks the row does not have
    // An open fan of more than NB entries keeps its LAST block in register position NB - 1 and its middle blocks NB - 1 ..
    // n - 2 in the pool: u_first and u_last, which the walk's telescoped antisymmetric part needs, are then always register
    // entries (the on-chip kernel moves the row's last ring entry into position NB - 1 to match).
    const bool open_long = !closed && n > NB;
    auto place = [&](int32_t j, double v0, double v1, double v2, uint32_t id) {
        if (open_long && j >= NB - 1) j = j == n - 1 ? NB - 1 : j + 1;
        emit(j, v0, v1, v2, id);
    };
    if (n < 2) {
        if (nblk == 1) emit(0, 0.0, 0.0, 0.0, 0u); // one entry, no triangle
        return;
    }
    auto entry = [&](int32_t k) {
        const uint32_t ww = P.ell16[tm.ell_off + lt + (int64_t)(k >> 1) * B];
        return (k & 1) ? (ww >> 16) : (ww & 0xffffu);
    };
    auto xy_of = [&](uint32_t lid) -> double2 {
        if (lid < (uint32_t)B) {
            const int64_t g = (int64_t)t * B + lid;
            return g < P.N ? P.xyP[g] : make_double2(0.0, 0.0);
        }
        return P.halo_xy[tm.hoff + (int32_t)(lid - B)];
    };
    const double2 ca = P.xyP[nd];
    const double2 z = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
    const uint32_t id0 = entry(0) & 0xfffu;
    double2 pd;
    {
        const double2 cxy = xy_of(id0);
        pd = make_double2(cxy.x - ca.x, cxy.y - ca.y);
    }
    double k0[3] = {0.0, 0.0, 0.0};    // block 0, held to the end
    double carry[3] = {0.0, 0.0, 0.0}; // K_ac of the triangle before entry k - 1: the first term of block k - 1
    uint32_t idprev = id0;
    for (int32_t k = 1; k < n; ++k) {
        const uint32_t id = entry(k) & 0xfffu;
        const double2 cxy = xy_of(id);
        const double2 d = make_double2(cxy.x - ca.x, cxy.y - ca.y);
        const double twoA = fma(pd.x, d.y, -(d.x * pd.y));
        const double wt = P.c0 * fast_rcp(twoA);
        double b00 = 0.0, b10 = 0.0, b01 = 0.0, b11 = 0.0, c00 = 0.0, c10 = 0.0, c01 = 0.0, c11 = 0.0;
        fan_force_w<double2, double>(pd, ex, d, z, wt, P.nu, P.h, b00, b10); // K_ab, first column
        fan_force_w<double2, double>(pd, ey, d, z, wt, P.nu, P.h, b01, b11);
        fan_force_w<double2, double>(pd, z, d, ex, wt, P.nu, P.h, c00, c10); // K_ac
        fan_force_w<double2, double>(pd, z, d, ey, wt, P.nu, P.h, c01, c11);
        const double bs = 0.5 * (b01 + b10), cs = 0.5 * (c01 + c10);
        if (k == 1) { // block 0 = K_ab of triangle 1 (+ K_ac of the closing triangle, below)
            k0[0] = 0.0 + b00;
            k0[1] = 0.0 + bs;
            k0[2] = 0.0 + b11;
        } else {
            place(k - 1, carry[0] + b00, carry[1] + bs, carry[2] + b11, idprev);
        }
        carry[0] = 0.0 + c00;
        carry[1] = 0.0 + cs;
        carry[2] = 0.0 + c11;
        pd = d;
        idprev = id;
    }
    if (closed) { // the last triangle closes onto entry 0
        place(0, k0[0] + carry[0], k0[1] + carry[1], k0[2] + carry[2], id0);
    } else {
        place(0, k0[0], k0[1], k0[2], id0);
        place(n - 1, carry[0], carry[1], carry[2], idprev);
    }
}

typedef void (*EdgeBlocksKernel)(const PersistParams, double *);
template <bool VAR>
static EdgeBlocksKernel edge_blocks_kernel(int32_t B, bool ovf)
{
    if (ovf) return B == 256 ? k_edge_blocks_ovf<256, VAR> : k_edge_blocks_ovf<512, VAR>;
    return B == 256 ? k_edge_blocks<256, VAR> : k_edge_blocks<512, VAR>;
}

// variants == 0: the blocks of the one operator of P into `kblocks`; variants >= 1: of so many variants in one launch
// (grid.y = variant), into P.kblocks (+ P.ovf_rec) at the var_* extents
void edge_blocks_build(const PersistParams &P, int32_t B, double *kblocks, int eb_mode, int32_t variants, hipStream_t s)
{
    const bool var = variants > 0;
    if (var && P.nranks > 1) return; // (variants run on one GPU)
    const int64_t npad = (int64_t)(P.nranks > 1 ? P.t1 - P.t0 : P.T) * B; // several ranks: this rank's own tiles
    const dim3 g((unsigned)((npad + 255) / 256), var ? (unsigned)variants : 1u);
    const EdgeBlocksKernel k = !var ? edge_blocks_kernel<false>(B, eb_mode == 2) : edge_blocks_kernel<true>(B, eb_mode == 2);
    k<<<g, 256, 0, s>>>(P, var ? nullptr : kblocks);
}

int persist_stamp_words() { return kStampPhases + 1; }
bool persist_stamps_built()
{
#ifdef MAG_PERSIST_STAMPS
    return true;
#else
    return false;
#endif
}

// bit 3 of the node mask, for the on-chip kernel with `k` tiles per workgroup: some tile of THIS rank's range [t0, t1) reads
// the node THROUGH MEMORY -- a tile of another workgroup, or a sibling tile whose rows do not all fit the registers (it
// keeps its halo copies).  One block per reading tile.  (Tiles of other ranks read through the inboxes, not through this
// GPU's granules: they mark nothing here.)
__global__ void __launch_bounds__(256) k_mark_external(const int32_t *halo_g, const TileMeta *meta, int32_t B, int32_t k,
                                                       int32_t max_reg_entries, int32_t t0, int32_t t1, uint8_t *maskP)
{
    const int32_t t = t0 + (int32_t)blockIdx.x;
    const TileMeta tm = meta[t];
    for (int32_t h = threadIdx.x; h < tm.nh; h += 256) {
        const int64_t g = halo_g[tm.hoff + h];
        const int32_t ot = (int32_t)(g / B);
        const bool sibling = ot >= t0 && ot < t1 && (ot - t0) / k == (t - t0) / k && tm.ent <= max_reg_entries;
        if (!sibling) atomicOr((unsigned int *)(maskP + (g & ~(int64_t)3)), 8u << (8 * (g & 3)));
    }
}

void mark_external(const int32_t *halo_g, const TileMeta *meta, int32_t t0, int32_t t1, int32_t B, int32_t k, uint8_t *maskP,
                   bool all_rows, hipStream_t s)
{
    if (t1 > t0)
        k_mark_external<<<t1 - t0, 256, 0, s>>>(halo_g, meta, B, k, all_rows ? 0x7fffffff : 2 * kPersistRegs, t0, t1, maskP);
}

// bit 2 of the node mask: some tile reads this node through its halo list, so its owner must publish q
__global__ void __launch_bounds__(256) k_mark_published(const int32_t *halo_g, int64_t halo_total, uint8_t *maskP)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= halo_total) return;
    // byte-wide atomic OR does not exist; neighbouring bytes belong to other nodes, so OR the containing word
    const int64_t g = halo_g[i];
    atomicOr((unsigned int *)(maskP + (g & ~(int64_t)3)), 4u << (8 * (g & 3)));
}

void mark_published(const int32_t *halo_g, int64_t halo_total, uint8_t *maskP, hipStream_t s)
{
    if (halo_total > 0) k_mark_published<<<(unsigned)((halo_total + 255) / 256), 256, 0, s>>>(halo_g, halo_total, maskP);
}


} // namespace magk
