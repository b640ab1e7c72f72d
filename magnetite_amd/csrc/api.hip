// C ABI of include/magnetite_hip.h: context, device buffers, phase
// orchestration of solver::run (solver.rs:543-586) on one MI355X.
// No CPU fallback exists: without a HIP device every compute entry point
// returns MAG_ERR_HIP with the runtime's message.
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <array>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "comm.h"
#include "kernels.h"
#include "magnetite_hip.h"
#include "primitives.h"
#include "adjoint.h"
#include "modal.h"
#include "modal_host.h"
#include "buckling.h"
#include "objective.h"
#include "design.h"
#include "recover.h"
#include "refine.h"
#include "sens.h"
#include "transient.h"
#include "explicit.h"
#include "explicit_tl.h"
#include "newton.h"
#include "transient_tl.h"

using magk::CgState;

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + (bytes >> 4) + 256; // a little slack: sizes that depend on the mesh grow slowly
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); } // every buffer of a mag_ctx goes with it (mag_destroy selects the device first)
    template <class T>
    T *as() const { return (T *)p; }
};

// What a set of solves on ONE uploaded mesh owns (load cases, design variants): `count` members, member after member in every
// buffer -- inputs, the uploaded problem while it is lent to a member that runs alone (keep), right-hand sides and solutions
// (Hilbert numbering), results (caller numbering) --, every member's statistics and the four words of mag_get_*_info.  An
// adjoint set (mag_run_adjoint) is one more of them per enum mag_set value: u_in = 0, f_in = dJ/du, solved by the hooks of
// the set whose members it differentiates.
struct MemberSet {
    const char *noun;   // in messages: "load case" / "variant"
    const char *run_fn; // the entry point that solves the set
    int32_t slot;       // enum mag_set: whose sensitivities and adjoint results a run of this set drops
    bool adjoint = false;
    int32_t count = 0;
    bool have = false, have_run = false;
    DevBuf uin, fin, keep, bP, x, u, f, stress;
    std::vector<mag_stats> stats;
    int32_t info[4] = {};
    void reset() // the set belongs to the mesh and mask it was given for
    {
        have = have_run = false;
        count = 0;
    }
};

// What a subspace iteration (subspace_iteration: mag_run_modal, mag_run_buckling) owns: the q vectors of the subspace as one more
// member set (u_in = 0, f_in = Y, solved as load cases are and, like an adjoint set, dropping nothing); the rotated vectors x (the
// shapes, at the end), w = the second operator on Z, the rotation's second Y, the residual vectors, the Gram partials, and Q, the
// values, the Gram matrices and the norms in `small`; the results on the host.
struct SubspacePass {
    MemberSet set;
    DevBuf x, w, y2, r, part, small, bad;
    bool have = false;
    int32_t info[8] = {};
    std::vector<double> lambda, residual;
    SubspacePass(const char *noun, const char *fn) : set{noun, fn, MAG_SET_CASES, true} {}
    void reset()
    {
        set.reset();
        have = false;
    }
};

// What a pass over the solved members of one set (enum mag_set) leaves -- mag_run_sensitivities, mag_run_adjoint (next to its
// adjoint MemberSet: lambda = that set's u, the adjoint reactions its f, dJ/du its f_in), mag_run_objective, mag_run_stress: its
// rows member after member on the device, the scalars on the host.  Dropped by a new mag_upload and by a new run of the set.
struct DerivedSet {
    bool have = false;
    bool totals = false; // mag_run_objective with_adjoint: dxy and scalars 4..7 hold the total derivatives
    int32_t count = 0;
    DevBuf energy;        // sensitivities [count][E]
    DevBuf dloads, delem; // adjoint [count][2N], [count][E]
    DevBuf g, pxy;        // objective [count][2N] each
    DevBuf selem, snode, seta2; // stress recovery [count][E][4], [count][N][4], [count][E]
    DevBuf dxy;           // the three design passes [count][2N]
    DevBuf scalars;       // every pass [count][8]
    std::vector<double> scalars_h;
};
enum Pass { PASS_SENS, PASS_ADJOINT, PASS_OBJECTIVE, PASS_STRESS, PASS_COUNT }; // the passes that leave a DerivedSet per set

// Run-time knobs (environment, read at every call: tests switch them between calls in one process).  None is needed in
// production; each one either is set by a test or forces a path the library can take on its own.
//   MAG_TUNE_FORCE_DIST=1                one rank runs the distributed protocol (tests/dist_worker.py: rccl1 rehearsal)
//   MAG_TUNE_SHARD_ORDER=0               several ranks build the whole mesh's tables (replicated ordering phase; tests)
//   MAG_TUNE_PERSIST_K=k                 at least k tiles per on-chip workgroup: ranks sharing one GPU co-resident (tests)
//   MAG_TUNE_PERSIST_MIN_K=k             small meshes / 256-node tiles reach the on-chip kernel (tests)
//   MAG_TUNE_PERSIST_SPIN=n              the on-chip kernel's spin budget (0 forces its fall-back; tests)
//   MAG_TUNE_PERSIST_TRIANGLES=1         the triangle walk where the mesh qualifies for edge blocks (tests)
//   MAG_TUNE_PERSIST_MG_BLOCKS=0         several ranks: the triangle walk instead of edge blocks (tests)
//   MAG_TUNE_PERSIST_MG_OVERFLOW=0       several ranks: the triangle walk instead of overflow records (tests)
//   MAG_TUNE_PERSIST_NO_OVERFLOW=1       a row of more than six blocks sends the mesh to the triangle walk (tests)
//   MAG_TUNE_PERSIST_FORCE_OVERFLOW=1    a structured mesh through the overflow instantiation (tests)
//   MAG_TUNE_PERSIST_STAMPS=<file>       stamped build only: the on-chip kernel's phase times (scripts/persist_phases.py)
//   MAG_TUNE_STREAM_SPIN=n               k_stream_exchange's spin budget (0 forces the all-reduce fall-back; tests)
//   MAG_TUNE_STREAM_INBOX=0              the all-reduce although inboxes are open: the only way past them on multi-GPU hardware
//   MAG_TUNE_ASSEMBLY=tiles|ctile        numeric assembly: k_assemble_tiles / k_assemble_fan where it fits (tests)
//   MAG_TUNE_PATTERN_SORT=1              the sort-based CSR pattern, the fall-back for rows of valence >= 16 (tests)
//   MAG_TUNE_GRID, MAG_TUNE_DMA          streaming kernels: grid cap, LDS-DMA staging off (cg.hip; tests)
//   MAG_TUNE_SENS_CHUNK=n                members per launch of the sensitivity kernels (tests; default: a device-memory bound)
//   MAG_TUNE_SENS_STAGE=0                the node kernel gathers from memory as on tiles too large for the LDS (tests)
//   MAG_TUNE_NEWTON_TIMES=<file>         mag_run_newton appends the run's phase times to <file> (scripts/newton_probe.py)
//   MAG_TUNE_TRANSIENT_TL_TIMES=<file>   mag_run_transient_tl appends the run's phase times to <file> (scripts/transient_tl_probe.py)
//   MAG_LIB_PATH                         Python binding: load another build of this library (magnetite_amd/_lib.py)
int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

int ceil_log2(int64_t n)
{
    int b = 0;
    while ((int64_t(1) << b) < n) ++b;
    return b < 1 ? 1 : b;
}

} // namespace

struct mag_ctx {
    mag_options opt;
    std::string err;
    bool hip_ok = false;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[10] = {};
    hipEvent_t evPoll[2] = {};
    CgState *h_state = nullptr; // pinned, 2 slots + final

    // problem (caller numbering)
    int64_t N = 0, E = 0;
    double youngs = 0, nu = 0, thick = 0;
    int32_t law = MAG_LAW_SVK; // mag_set_material_law: the material of the total-Lagrangian passes; kept across uploads
    bool have_problem = false, have_order = false, have_csr = false, have_run = false;
    // (perm, the incidence lists, the tiles and their halo lists hang on the connectivity and the uploaded coordinates only: they
    // outlive have_order, which a variants run drops because xyP and K may be a variant's)
    DevBuf xy, conn, uknown, uin, fin;

    // ordering / tiles
    int32_t B = 512, T = 0;
    int bitsN = 1;
    int64_t ell_total = 0;
    DevBuf scratch, small; // rocPRIM temp; small = bbox partials, bbox, err flag
    DevBuf sK0, sK1, sV0, sV1;
    DevBuf perm, iperm, xyP, maskP, deg, inc_off, inc, tile_deg, tile_rdeg, tile_cnt, tile_off, ell, ell_asm, ell_pos;
    DevBuf bc_touch; // N bytes: rows with a prescribed column (k_pattern_rows; k_mark_bc_rows on the sort-based pattern)
    bool bc_touch_ready = false;
    DevBuf kblocks; // on-chip CG, edge-block instantiation: the nodes' blocks (k_edge_blocks)
    DevBuf row_info, ovf_cnt, ovf_off, ovf_rec; // ... with overflow: k_ring16's per-row byte, per-node counts, their scan, the records
    bool asm_ctile = false; // K is assembled from the CG tiles (k_assemble_fan), ell_asm holds its corner words
    // tile-local numbering for the LDS-halo operator
    bool use_lds = false;
    int32_t cap = 0, max_halo = 0;
    int64_t halo_total = 0;
    DevBuf hcnt, hoffn, hk0, hk1, halo_g, halo_xy, tile_hcnt, tile_hoff;
    // multi-GPU partition: this rank owns tiles [t0,t1) = nodes [own0,own1) of the Hilbert order
    int32_t t0 = 0, t1 = 0, own0 = 0, own1 = 0, n_iface = 0;
    bool dist = false; // CG runs the distributed protocol (nranks > 1, or forced for a 1-rank rehearsal)
    DevBuf iface, comm_pq, comm_rr, gath_send, gath_recv;

    // CSR of K (caller numbering)
    int64_t nb = 0;
    DevBuf pk0, pk1, pv0, pv1, head, blk, rowcnt, seg_start, bptr, brow, bcol, kval, ke;
    // multi-GPU: a rank keeps only the K rows of its own nodes, one ghost layer and the prescribed nodes
    bool csr_full = true;    // the CSR held now covers every row (one rank, or a test entry point asked for all of K)
    bool want_full_csr = false; // mag_assemble_csr / mag_reduce_system on a multi-rank context: build all of K
    DevBuf local_node, ecnt, eoff;
    // several ranks: the ordering phase's per-tile tables for the tiles this rank needs only (need_tile), decided per run
    DevBuf need_tile, iface_mask;
    bool order_sharded = false, order_allow_shard = false;
    int32_t fan_flags_global = 3;
    // reduced system scratch
    DevBuf isfree, fidx, rcnt, rowoff, rp_ff, col_ff, val_ff, b_ff, rp_full, col_full;
    int64_t nf = 0, nz_ff = 0;

    // CG (Hilbert numbering)
    DevBuf x, r, p0, p1, q, bP, tmpP, partRR, partPQ, state, hist;
    // fused single-launch variant
    DevBuf rqp0, rqp1, fpart, fstate, tmeta, comm_f, own_qslot, halo_qslot, minvP, halo_minv;
    magk::FusedState *h_fstate = nullptr; // pinned, 3 slots
    bool fused = false;
    int32_t fgrid = 1; // workgroups of the fused kernel for this problem
    int32_t g_all = 1; // ... of the rank with the most tiles: dot-partial slots of the exchange buffer (multi-GPU)
    size_t cwords = 0; // doubles per exchange buffer: nsums * g_all + 2 * n_iface
    bool pre = false;  // mag_options.preconditioner != 0
    // on-chip CG (persist_kernel.h, k_cg_persist): the whole solve in one launch when every tile fits registers + LDS
    bool persist = false, persist_failed = false;
    // after a grid-barrier timeout the context streams for `persist_retry_in` solves, then tries the on-chip kernel again;
    // the wait doubles with every further failure (8 .. 1024 solves) and starts over after a success
    int persist_backoff = 0, persist_retry_in = 0;
    int32_t persist_k = 0, persist_grid = 0, persist_maxh = 0, cg_kernel = 0;
    DevBuf qx, wg_part, psync, grec; // published-q granules, partial-record granules, timeout word, republished sums
    // multi-GPU on-chip CG: a window of host memory mapped by every rank (mag_comm_set_window)
    void *win_host = nullptr, *win_dev = nullptr;
    size_t win_bytes = 0;
    // ... or, better, one inbox per rank in DEVICE memory, IPC-mapped by the others (mag_comm_inbox_*)
    void *inbox_own = nullptr, *inbox_peer[8] = {};
    bool inbox_peer_local[8] = {}; // the peer's inbox lives in THIS process (ranks as threads): a plain pointer, not an IPC mapping
    std::array<uint8_t, MAG_IPC_HANDLE_BYTES> inbox_handle = {};
    size_t inbox_bytes = 0;
    bool inbox_ready = false;
    DevBuf iface_readers;
    uint32_t solve_seq = 0;
    double best_cost = 0.0;   // argmin's best_param bookkeeping, as the CG phase that just ran reported it
    long long best_iter = 0;
    // the on-chip kernel gave up at its grid barrier / an inbox exchange gave up in this run (mag_stats.persist_timeout /
    // exchange_timeout)
    bool persist_timed_out = false, exchange_timed_out = false;
    bool b_from_order = false; // the ordering phase of this run wrote b = 0.0 + f for every node (k_apply_order)
    int edge_blocks = 0; // instantiation of the on-chip kernel of the last run: 1 edge blocks, 2 with overflow records (mag_stats.edge_blocks)
    // streaming kernels across GPUs: the per-iteration exchange through the device inboxes (k_stream_exchange) instead of
    // an all-reduce; si_failed: a wait ran out once, this context uses the all-reduce from then on
    bool si = false, si_failed = false;
    uint32_t si_tag_base = 0, si_spin = 1u << 20; // polls (~2 us each) before an exchange gives up
    int32_t exchange_kind = 0; // mag_stats.exchange of the last run
    int nsums() const { return pre ? 5 : 4; }
    DevBuf pstamps; // diagnostic build of the on-chip kernel: phase stamps
    DevBuf xy32, hxy32, rqp32a, rqp32b, x32; // fp32 leg (mag_options.precision = 1)
    hipGraphExec_t graph = nullptr;
    struct GraphKey {
        void *ptrs[20];
        int64_t N;
        int32_t T, B, G, hist_len;
        void *dptrs[12];  // distributed block (streaming kernels + k_stream_exchange): exchange buffer, slot tables, inboxes
        int32_t d[12];    // ... and its scalars (all zero on one GPU)
    } gkey = {};

    // results (caller numbering)
    DevBuf u, f, stress;
    mag_stats stats = {};

    // load cases (mag_set_load_cases / mag_run_cases): sets of prescribed values on the uploaded mesh; design variants
    // (mag_set_variants / mag_run_variants): shapes / materials / value sets of it (variants.uin / fin only when given).  Two
    // sets: load cases survive a variants run
    MemberSet cases{"load case", "mag_run_cases", MAG_SET_CASES}, variants{"variant", "mag_run_variants", MAG_SET_VARIANTS};
    // the on-chip kernel's granules, records, timeout words and states for the members of ONE launch, of either set
    DevBuf launch_qx, launch_part, launch_sync, launch_state;

    // what only variants have.  Inputs variant after variant (v_xy only when given; v_mat: E, nu, thickness; v_cmat: the CG
    // kernels' c0, nu, h); the per-variant OPERATOR data -- permuted coordinates, K values, edge blocks, overflow records --
    // for the variants of ONE chunk only
    bool v_have_xy = false, v_have_loads = false;
    DevBuf v_xy, v_mat, v_cmat, v_bad;
    DevBuf v_xyP, v_halo, v_kval, v_kblocks, v_ovf;
    std::vector<double> v_mat_h; // [variants.count][3] = E, nu, thickness
    int32_t ovf_total = 0; // overflow records of the whole mesh (choose_edge_blocks)
    hipEvent_t evV[7] = {}; // phase boundaries of a chunk (created by the first mag_run_variants)

    // what the passes over solved members left of the last mag_run, mag_run_cases, mag_run_variants: [enum Pass][enum mag_set]
    DerivedSet derived[PASS_COUNT][3];

    // energy and design sensitivities (mag_run_sensitivities): the materials, per-element nu terms and partial sums of ONE chunk
    // of members
    DevBuf sens_mat, sens_nuterm, sens_part, sens_tab; // sens_tab: the node kernel's tile-local corner table, of this ordering
    bool sens_tab_ready = false;

    // adjoint sensitivities (mag_run_adjoint) of the same three sets: the adjoint systems as member sets of their own (what the
    // bilinear pass made of them is derived[PASS_ADJOINT]), and the single-case results kept aside while the adjoint systems run
    MemberSet adj[3] = {{"adjoint", "mag_run_adjoint", MAG_SET_RUN, true},
                        {"adjoint", "mag_run_adjoint", MAG_SET_CASES, true},
                        {"adjoint", "mag_run_adjoint", MAG_SET_VARIANTS, true}};
    DevBuf adj_keep;

    // objectives of the same three sets (mag_run_objective); the caller's weights and targets, and the summands, per-element
    // factors and member factors of ONE chunk of members (the nu terms and partial sums are the sensitivities')
    DevBuf obj_w, obj_target, obj_terms, obj_helem, obj_factor;

    // modal analysis (mag_run_modal): the state of its subspace iteration (SubspacePass) -- f_in = Y = M X, W = M Z, the values are
    // the eigenvalues.  The results hang on the upload only: a new mag_upload drops them, a new mag_run_modal replaces them
    SubspacePass modal{"mode vector", "mag_run_modal"};

    // linearised buckling (mag_run_buckling): the same state once more -- f_in = Y = -K_G X, the values are the load factors -- and
    // the prestress u0, copied from the solved member before the first inner solve (the inner solves run through the context's
    // own vectors); bk_kg: mag_assemble_geometric's values.  A new mag_upload drops the results, a new mag_run_buckling replaces them
    SubspacePass buckling{"buckling vector", "mag_run_buckling"};
    DevBuf bk_u0, bk_kg;

    // mesh refinement (mag_run_refine): the tables of the pass (rf_tab: one allocation, carved up per call), the caller's marks
    // or indicator while they are read, rocPRIM's temporary of its sorts and scans (its own: the ordering phase's stays as it is),
    // and the refined mesh with its parents, which outlives mag_upload_refined.  A caller's mag_upload drops it
    DevBuf rf_tab, rf_in, rf_tmp, rf_xy, rf_conn, rf_uknown, rf_uin, rf_fin, rf_nparents, rf_eparent;
    bool rf_have = false;
    int64_t rf_info[8] = {};

    // element stiffness field (mag_set_element_scale): E relative scales on the device while field_on.  field_sym: the order, the
    // tables and the CSR pattern held now were built under this field (with the CSR operator's choices) and a run keeps them
    DevBuf escale;
    bool field_on = false, field_sym = false;
    // mag_options.field_cg: the tile-local block-row table of K (k_field_rows: per tile meta, slots, sources -- of this order and
    // this pattern, dropped with either), the values gathered from kval after every assembly, the workgroups of k_cg_field
    DevBuf fc_width, fc_meta, fc_slot, fc_src, fc_val;
    bool fc_ready = false;
    int64_t fc_total = 0;
    int32_t fc_grid = 1;
    double fc_build_ms = 0.0; // the table was built in this run: its time (mag_stats.ms_csr_symbolic)

    // density design (mag_design_init / mag_design_step): the densities, the filter's tables and the update's scratch; the
    // bracket, the sums and the info words live on the device between the launches of a step
    bool design_on = false;
    mag_design_options design_opt = {};
    int64_t design_steps = 0;
    double design_info[8] = {};
    DevBuf ds_rho, ds_rhof, ds_w, ds_area, ds_node_area, ds_node, ds_tmp, ds_dJ, ds_dJdrho, ds_bq, ds_rho_new, ds_part, ds_small;

    // What the passes on the assembled pattern share, none of it a result (mag_run_transient, mag_run_explicit, mag_run_newton,
    // mag_run_transient_tl and the single evaluations).  ptab: the block-row table of K's pattern, the gathered values of the
    // pass's matrix and the inverse blocks, in buffers of the passes' own (fc_* are a field's, kept between runs): every run
    // rebuilds the table and regathers the values before its first solve, nothing is carried between runs in it.  chk_words,
    // chk_probes: the 16 bytes of the device checks (StepWords) and the probe list of the run in flight.  ev_u, ev_words: the state
    // and the words (EvalWords) of mag_internal_force, mag_assemble_tangent and mag_assemble_effective_tangent
    struct PassTable {
        DevBuf width, meta, slot, src, val, minv, hminv;
    } ptab;
    DevBuf chk_words, chk_probes, ev_u, ev_words;

    // transient dynamics (mag_run_transient): the mass and the effective matrix in K's pattern (tr_aval in kval's layout), the
    // state, the predictors, the right-hand side, a zero vector, the records of the last run, and the words of
    // mag_get_transient_info.  The results hang on the upload only: a new mag_upload drops them, a new run replaces them
    DevBuf tr_mval, tr_aval;
    DevBuf tr_u, tr_v, tr_a, tr_ut, tr_vt, tr_rhs, tr_zero, tr_f, tr_ku, tr_mv, tr_amp, tr_in;
    DevBuf tr_probe, tr_energy, tr_snap, tr_part;
    bool tr_have = false;
    int32_t tr_info[8] = {}, tr_steps = 0, tr_num_probes = 0, tr_snaps = 0;
    bool tr_energies = false;
    double tr_t0 = 0.0, tr_t1 = 0.0, tr_amp_last = 1.0;
    std::vector<int32_t> tr_iterations;
    // the length of the FIRST poll block of the pass's next solve (0: check_every, as for every other caller): the pass expects
    // the iteration count of its previous solve and polls in short blocks behind it
    int32_t tr_first_block = 0;
    // explicit dynamics (mag_run_explicit) leaves its final state and its records in the transient pass's slots (either pass
    // resumes the other's state; mag_download_transient serves both).  tr_rows: the record rows of the last run of either pass;
    // tr_dt, tr_dt_bound: scalars[2..3] (0 after the implicit pass).  Its own buffers: the state records in Hilbert order (two:
    // a step reads one and writes the other), the node masses, u_in and f_in in Hilbert order, the bound's partials and result;
    // its flags are in chk_words once the checks are read back
    DevBuf ex_rec[2], ex_mass, ex_uin, ex_f, ex_part, ex_out;
    // mag_internal_force's own buffers (it changes no result of the context): f_int(u), the energy's partials
    DevBuf tl_f, tl_part;
    int64_t tr_rows = 0;
    double tr_dt = 0.0, tr_dt_bound = 0.0;

    // nonlinear statics (mag_run_newton): the tangent in K's pattern (nt_kval in kval's layout), the state and its trial, the last
    // converged state, the step and its support part, a zero vector, f_int, the right-hand side, the results, the device's
    // records and the scalars of an evaluation; the records the host keeps; the words of mag_get_newton_info.  The results hang on
    // the upload only: a new mag_upload drops them, a new run replaces them
    DevBuf nt_kval;
    DevBuf nt_u, nt_ut, nt_uc, nt_du, nt_dup, nt_zero, nt_f, nt_rhs, nt_fout, nt_elem, nt_load, nt_probe, nt_snap, nt_part, nt_scal;
    bool nt_have = false;
    int32_t nt_info[8] = {}, nt_increments = 0, nt_num_probes = 0, nt_snaps = 0;
    std::vector<double> nt_loads, nt_energies, nt_residuals, nt_steps;
    std::vector<int32_t> nt_newton, nt_cg;

    // nonlinear transient dynamics (mag_run_transient_tl): the effective tangent in K's pattern (tt_aval in kval's layout), the
    // trial state (a', u', v'), the Newton step, f_int, the element rows, the scalars of an iteration, the partials; the records
    // the host keeps; the words of mag_get_transient_tl_info.  The final state and the step records are in the transient pass's
    // slots (tr_*)
    DevBuf tt_aval;
    DevBuf tt_an, tt_un, tt_vn, tt_da, tt_fint, tt_elem, tt_scal, tt_part, tt_move;
    bool tt_have = false;
    int32_t tt_info[8] = {};
    std::vector<double> tt_residuals;
    std::vector<int32_t> tt_newton, tt_cg;

    magc::Comm comm;
};

namespace {

int fail(mag_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(call)                                                                                       \
    do {                                                                                                   \
        const hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess)                                                                              \
            return fail(ctx, MAG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                         \
    } while (0)

int enter(mag_ctx *ctx)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!ctx->hip_ok) return MAG_ERR_HIP; // message was set by mag_create
    HIPCHK(hipSetDevice(ctx->device));
    return MAG_OK;
}

// K is assembled: asked for, or the CG operator is its CSR
inline bool wants_csr(const mag_ctx *ctx) { return ctx->opt.assemble_csr != 0 || ctx->opt.cg_operator == MAG_OP_CSR; }

// ---- the element stiffness field (mag_set_element_scale)
// what does not honour a field refuses it by name, before any HIP call
int field_refuses(mag_ctx *ctx, const char *fn)
{
    return fail(ctx, MAG_ERR_STATE, "%s: not available while an element stiffness field is set (mag_set_element_scale; NULL clears it)", fn);
}

// the contexts a field cannot be set on, or run under: again before any HIP call
int field_context_refused(mag_ctx *ctx, const char *fn)
{
    const char *why = ctx->comm.nranks > 1            ? "a communicator of more than one rank"
                      : ctx->opt.assemble_csr == 0    ? "assemble_csr = 0 (the field lives in the assembled K)"
                      : ctx->opt.precision == 1       ? "precision = 1 (the fp32 leg is matrix-free)"
                      : ctx->opt.preconditioner != 0  ? "a preconditioner (it needs the fused matrix-free iteration)"
                                                      : nullptr;
    return why ? fail(ctx, MAG_ERR_STATE, "%s: an element stiffness field does not work with %s", fn, why) : MAG_OK;
}

// While a field is set the CG runs the CSR operator's phase whatever mag_options.cg_operator says (the on-chip kernel's edge
// blocks and the matrix-free operators assume one material): the option reads MAG_OP_CSR for the length of a call.
struct FieldOperator {
    mag_ctx *ctx;
    const int32_t cg_operator;
    // (force: mag_design_init builds the order of the field it is about to install)
    explicit FieldOperator(mag_ctx *c, bool force = false) : ctx(c), cg_operator(c->opt.cg_operator)
    {
        if (ctx->field_on || force) ctx->opt.cg_operator = MAG_OP_CSR;
    }
    ~FieldOperator() { ctx->opt.cg_operator = cg_operator; }
};
inline const double *field_of(const mag_ctx *ctx) { return ctx->field_on ? ctx->escale.as<double>() : nullptr; }
// mag_options.field_cg: under a field the CG runs the fused block-row phase (cg_phase_field) where the context has the
// tile-local tables; without them (op_variant 1, a tile beyond LDS) the CSR operator's phase runs as before.  Valid once the
// order is there.
inline bool field_cg_selected(const mag_ctx *ctx) { return ctx->field_on && ctx->opt.field_cg != 0 && ctx->use_lds; }
// the CG phase of this context leaves its solution expanded in ctx->u (the CSR operator's), not in ctx->x in Hilbert numbering
inline bool solution_expanded(const mag_ctx *ctx) { return ctx->opt.cg_operator == MAG_OP_CSR && !field_cg_selected(ctx); }
inline bool memory_known(int32_t memory) { return memory == MAG_MEM_HOST || memory == MAG_MEM_DEVICE; }
// The one rule of the ABI: a `memory` that is none of enum mag_memory is refused where a pointer it describes would be read or
// written, among the argument checks that precede any HIP call (fn: the entry point, named in the message)
int memory_refused(mag_ctx *ctx, int32_t memory, const char *fn)
{
    if (memory_known(memory)) return MAG_OK;
    return fail(ctx, MAG_ERR_BAD_ARGS, "%s: memory = %d is none of enum mag_memory", fn, (int)memory);
}
// the copies into a caller's buffers of kind `memory`: from the device, from the host
struct OutKinds {
    hipMemcpyKind dev, host;
};
inline OutKinds out_kinds(int32_t memory)
{
    const bool d = memory == MAG_MEM_DEVICE;
    return {d ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, d ? hipMemcpyHostToDevice : hipMemcpyHostToHost};
}
inline hipMemcpyKind in_kind_of(int32_t memory) { return memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }

// the two rules of the real-valued arguments, among the argument checks (what: the field, named in the message)
inline bool nonneg_finite(double x) { return x >= 0.0 && std::isfinite(x); }
inline bool pos_finite(double x) { return x > 0.0 && std::isfinite(x); }
using NamedValues = std::initializer_list<std::pair<const char *, double>>; // checked in the order given
int need_nonneg(mag_ctx *ctx, const char *fn, NamedValues fields)
{
    for (const auto &[what, x] : fields)
        if (!nonneg_finite(x)) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: %s %g is negative or not finite", fn, what, x);
    return MAG_OK;
}
int need_pos(mag_ctx *ctx, const char *fn, NamedValues fields)
{
    for (const auto &[what, x] : fields)
        if (!pos_finite(x)) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: %s %g is not positive and finite", fn, what, x);
    return MAG_OK;
}

int scratch_for(mag_ctx *ctx, size_t bytes)
{
    HIPCHK(ctx->scratch.reserve(bytes));
    return MAG_OK;
}

int sort_u32(mag_ctx *ctx, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n,
             int end_bit)
{
    size_t tb = 0;
    HIPCHK(magp::sort_pairs_u32(nullptr, &tb, kin, kout, vin, vout, n, 0, end_bit, ctx->stream));
    if (int rc = scratch_for(ctx, tb)) return rc;
    HIPCHK(magp::sort_pairs_u32(ctx->scratch.p, &tb, kin, kout, vin, vout, n, 0, end_bit, ctx->stream));
    return MAG_OK;
}

int sort_u64(mag_ctx *ctx, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, size_t n,
             int end_bit)
{
    size_t tb = 0;
    HIPCHK(magp::sort_pairs_u64(nullptr, &tb, kin, kout, vin, vout, n, 0, end_bit, ctx->stream));
    if (int rc = scratch_for(ctx, tb)) return rc;
    HIPCHK(magp::sort_pairs_u64(ctx->scratch.p, &tb, kin, kout, vin, vout, n, 0, end_bit, ctx->stream));
    return MAG_OK;
}

int scan_i32(mag_ctx *ctx, const int32_t *in, int32_t *out, size_t n)
{
    size_t tb = 0;
    HIPCHK(magp::exclusive_scan_i32(nullptr, &tb, in, out, n, ctx->stream));
    if (int rc = scratch_for(ctx, tb)) return rc;
    HIPCHK(magp::exclusive_scan_i32(ctx->scratch.p, &tb, in, out, n, ctx->stream));
    return MAG_OK;
}

int scan_i64(mag_ctx *ctx, const int64_t *in, int64_t *out, size_t n)
{
    size_t tb = 0;
    HIPCHK(magp::exclusive_scan_i64(nullptr, &tb, in, out, n, ctx->stream));
    if (int rc = scratch_for(ctx, tb)) return rc;
    HIPCHK(magp::exclusive_scan_i64(ctx->scratch.p, &tb, in, out, n, ctx->stream));
    return MAG_OK;
}

// ---- collectives of the multi-GPU paths ----
// in-place sum over ranks of n doubles at dev, ordered on the stream
int allreduce(mag_ctx *ctx, double *dev, int64_t n)
{
    std::string msg;
    if (int rc = ctx->comm.allreduce_sum(dev, n, ctx->stream, msg)) return fail(ctx, rc, "%s", msg.c_str());
    return MAG_OK;
}

int allgather(mag_ctx *ctx, const double *send, double *recv, int64_t n)
{
    std::string msg;
    if (int rc = ctx->comm.allgather(send, recv, n, ctx->stream, msg)) return fail(ctx, rc, "%s", msg.c_str());
    return MAG_OK;
}

// n host doubles summed over ranks through comm_pq (128 bytes); the host waits for the result
int allreduce_host(mag_ctx *ctx, double *v, int n)
{
    assert(n <= 16);
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(ctx->comm_pq.p, v, 8 * (size_t)n, hipMemcpyHostToDevice, s));
    if (int rc = allreduce(ctx, ctx->comm_pq.as<double>(), n)) return rc;
    HIPCHK(hipMemcpyAsync(v, ctx->comm_pq.p, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// what all ranks must decide alike: flag becomes true on every rank when it is true on any
int any_rank(mag_ctx *ctx, bool &flag)
{
    double v = flag ? 1.0 : 0.0;
    if (int rc = allreduce_host(ctx, &v, 1)) return rc;
    flag = v != 0.0;
    return MAG_OK;
}

// rank r owns tiles [rank_tile_lo(r), rank_tile_lo(r + 1)): contiguous ranges of the Hilbert order, identical arithmetic on
// every rank, equal up to one tile
int32_t rank_tile_lo(int64_t T, int R, int r) { return (int32_t)((T * r) / R); }

// the most tiles any rank runs: T mod R ranks get the ceiling
int32_t most_rank_tiles(int64_t T, int R) { return (int32_t)((T + R - 1) / R); }

// sequence number of a solve across ranks (1..255, the same on every rank: all ranks run the same solves), kept above 24
// bits of iteration count in the tags of the inbox exchanges
uint32_t next_solve_seq(mag_ctx *ctx)
{
    ctx->solve_seq = (ctx->solve_seq + 1) & 0xffu;
    if (ctx->solve_seq == 0) ctx->solve_seq = 1;
    return ctx->solve_seq;
}

// the material constants of the operator kernels (the fp32 leg rounds the fp64 values)
template <class Params>
void set_material(const mag_ctx *ctx, Params &P)
{
    using F = decltype(P.c0);
    P.c0 = (F)(ctx->youngs * ctx->thick / (2.0 * (1.0 - ctx->nu * ctx->nu)));
    P.nu = (F)ctx->nu;
    P.h = (F)((1.0 - ctx->nu) / 2.0);
}

// the material constants of the total-Lagrangian kernels (explicit_tl.h) under the context's law: St. Venant-Kirchhoff takes
// set_material's; neo-Hooke c0 = mu t / 2, nu = Lambda / mu, h unread
template <class Params>
void set_tl_material(const mag_ctx *ctx, Params &P)
{
    set_material(ctx, P);
    P.law = ctx->law;
    if (ctx->law == MAG_LAW_NEO_HOOKE) {
        P.c0 = ctx->youngs * ctx->thick / (4.0 * (1.0 + ctx->nu));
        P.nu = 2.0 * ctx->nu / (1.0 - 2.0 * ctx->nu);
        P.h = 0.0;
    }
}

// the factor of the element rows' stresses (newton_elements): E / (1 - nu^2), under neo-Hooke mu
double tl_stress_scale(const mag_ctx *ctx)
{
    return ctx->law == MAG_LAW_NEO_HOOKE ? ctx->youngs / (2.0 * (1.0 + ctx->nu)) : ctx->youngs / (1.0 - ctx->nu * ctx->nu);
}

// ---- symbolic phase 1: Hilbert order, incidence lists, per-tile ELL table ----
int ensure_order(mag_ctx *ctx)
{
    if (ctx->have_order) return MAG_OK;
    ctx->sens_tab_ready = false;
    ctx->fc_ready = false; // (the block-row table is of this order's tiles and halo lists)
    const int64_t N = ctx->N, E = ctx->E;
    // automatic tile size: 512-node tiles once the mesh has at least as many of them as the fused kernel keeps
    // resident (2 per CU x 256 CUs); smaller meshes are latency-bound and run faster on twice as many 256-node tiles
    // (measured: 100k triangles 6.6 vs 7.7 us per iteration; 1M triangles 22.0 vs 20.4)
    // (since the on-chip CG exists, 512-node tiles also win on mid-size meshes it can hold: 6.2 / 6.4 / 8.3 us per
    // iteration at 59k / 121k / 245k nodes against 6.9 / 8.8 / 13.8 with streamed 256-node tiles)
    const bool on_chip_candidate = ctx->opt.cg_variant == 2 &&
                                   (ctx->comm.nranks == 1 || ctx->win_dev != nullptr || ctx->inbox_ready) &&
                                   getenv("MAG_TUNE_FORCE_DIST") == nullptr && ctx->opt.precision == 0 &&
                                   ctx->opt.preconditioner == 0 && ctx->opt.cg_operator == MAG_OP_MATRIX_FREE &&
                                   ctx->opt.op_variant != 1 && !ctx->persist_failed;
    // (round 4: on ONE GPU the on-chip kernel takes every mesh it can hold, the small ones included -- the reference's own
    // examples are a few thousand triangles: 3.85 against 6.5 us per iteration for the streaming kernels replayed from a graph
    // at 1k-27k triangles, and no graph to instantiate in the first solve (scripts/small_mesh_probe.py); across ranks the lower
    // bound stays, so that every rank gets tiles)
    if (ctx->opt.tile_nodes == 0)
        ctx->B = (N >= 512 * 512 || (on_chip_candidate && (N >= 32768 || ctx->comm.nranks == 1) &&
                                     N <= (int64_t)ctx->comm.nranks * 1024 * 512))
                     ? 512 : 256;
    const int32_t B = ctx->B;
    const int32_t T = (int32_t)((N + B - 1) / B);
    ctx->T = T;
    ctx->bitsN = ceil_log2(N);
    hipStream_t s = ctx->stream;
    const size_t nmax = (size_t)(N > 3 * E ? N : 3 * E);
    HIPCHK(ctx->sK0.reserve(4 * nmax + 16));
    HIPCHK(ctx->sK1.reserve(4 * nmax + 16));
    HIPCHK(ctx->sV0.reserve(4 * nmax + 16));
    HIPCHK(ctx->sV1.reserve(4 * nmax + 16));
    HIPCHK(ctx->small.reserve(8 * (4 * 256 + 4) + 64)); // bbox partials, bbox, {error flag, known count}
    HIPCHK(ctx->perm.reserve(4 * (size_t)N));
    HIPCHK(ctx->iperm.reserve(4 * (size_t)N));
    HIPCHK(ctx->xyP.reserve(16 * (size_t)N));
    HIPCHK(ctx->maskP.reserve((size_t)N));
    HIPCHK(ctx->bP.reserve(16 * (size_t)N)); // written by apply_order (b = 0.0 + f), completed after the assembly
    HIPCHK(ctx->deg.reserve(4 * ((size_t)N + 1)));
    HIPCHK(ctx->inc_off.reserve(4 * ((size_t)N + 1)));
    HIPCHK(ctx->inc.reserve(4 * 3 * (size_t)E));
    HIPCHK(ctx->tile_deg.reserve(4 * ((size_t)T + 1)));
    HIPCHK(ctx->tile_cnt.reserve(8 * ((size_t)T + 1)));
    HIPCHK(ctx->tile_off.reserve(8 * ((size_t)T + 1)));

    double *part = ctx->small.as<double>();
    double *bbox4 = part + 4 * 256;
    int32_t *errflag = (int32_t *)(bbox4 + 4);

    magk::bbox(ctx->xy.as<double>(), N, part, bbox4, s);
    magk::hilbert_keys(ctx->xy.as<double>(), N, bbox4, ctx->sK0.as<uint32_t>(), ctx->sV0.as<uint32_t>(), s);
    if (int rc = sort_u32(ctx, ctx->sK0.as<uint32_t>(), ctx->sK1.as<uint32_t>(), ctx->sV0.as<uint32_t>(),
                          ctx->sV1.as<uint32_t>(), (size_t)N, 2 * magk::kHilbertBits))
        return rc;
    // perm = the sorted ids, every tile stably partitioned by valence class (round 4; the identity on structured meshes):
    // the on-chip kernel's long rows then share waves instead of being spread over all of them (symbolic.hip).  The
    // triangles per node it needs are counted in caller numbering (inc_off is free until the scan below) and carried into
    // the new numbering by apply_order: k_incidence_keys then counts nothing.
    bool counted = false;
    if (B == 256 || B == 512) {
        HIPCHK(hipMemsetAsync(ctx->inc_off.p, 0, 4 * ((size_t)N + 1), s));
        magk::count_degree(ctx->conn.as<int32_t>(), E, N, ctx->inc_off.as<int32_t>(), s);
        magk::tile_valence_partition(ctx->sV1.as<uint32_t>(), ctx->inc_off.as<int32_t>(), N, B, T, ctx->perm.as<uint32_t>(), s);
        counted = true;
    } else {
        HIPCHK(hipMemcpyAsync(ctx->perm.p, ctx->sV1.p, 4 * (size_t)N, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipMemsetAsync(errflag, 0, 8, s)); // {error flag, prescribed-displacement count}
    magk::apply_order(ctx->perm.as<uint32_t>(), ctx->xy.as<double>(), ctx->uknown.as<uint8_t>(), N,
                      ctx->iperm.as<int32_t>(), ctx->xyP.as<double>(), ctx->maskP.as<uint8_t>(), errflag + 1,
                      counted ? ctx->inc_off.as<int32_t>() : nullptr, ctx->deg.as<int32_t>(), ctx->fin.as<double>(),
                      ctx->bP.as<double>(), s);
    ctx->b_from_order = true;

    // ---- partition: contiguous tile ranges of the Hilbert order, identical arithmetic on every rank ----
    const int R = ctx->comm.nranks, me = ctx->comm.rank;
    ctx->t0 = rank_tile_lo(T, R, me);
    ctx->t1 = rank_tile_lo(T, R, me + 1);
    // (T < R, not "my range is empty": every rank must take this exit together -- the others would wait in a collective)
    if (R > 1 && T < R) return fail(ctx, MAG_ERR_BAD_ARGS, "mesh has %d tiles, fewer than %d ranks", (int)T, R);
    // Several ranks, inside mag_run (every rank is here: the phase then ends with two small all-reduces), K assembled from the
    // rows a rank keeps: the tables below are built for the tiles this rank needs only (symbolic.hip, need_tiles).  Any other
    // entry point -- and MAG_TUNE_SHARD_ORDER=0 -- builds them for the whole mesh, as every rank did until round 4.
    const bool csr_rows = wants_csr(ctx);
    const bool sh = R > 1 && ctx->order_allow_shard && csr_rows && !ctx->want_full_csr &&
                    env_int("MAG_TUNE_SHARD_ORDER", 1) != 0 && getenv("MAG_TUNE_FORCE_DIST") == nullptr;
    ctx->order_sharded = sh;
    if (!counted) HIPCHK(hipMemsetAsync(ctx->deg.p, 0, 4 * ((size_t)N + 1), s));
    if (sh) {
        HIPCHK(ctx->need_tile.reserve((size_t)T + 64));
        magk::RankTiles rt = {};
        rt.R = R;
        for (int r_ = 0; r_ <= R; ++r_) rt.lo[r_] = rank_tile_lo(T, R, r_);
        HIPCHK(ctx->iface_mask.reserve((size_t)N + 64));
        magk::need_tiles(ctx->conn.as<int32_t>(), E, ctx->iperm.as<int32_t>(), ctx->maskP.as<uint8_t>(), N, B, T, ctx->t0, ctx->t1,
                         true, ctx->need_tile.as<uint8_t>(), rt, ctx->iface_mask.as<uint8_t>(), s);
        if (counted) magk::zero_unneeded_deg(ctx->need_tile.as<uint8_t>(), N, B, ctx->deg.as<int32_t>(), s);
        magk::incidence_flags(ctx->conn.as<int32_t>(), E, ctx->iperm.as<int32_t>(), N, B, ctx->need_tile.as<uint8_t>(),
                              ctx->sK1.as<int32_t>(), errflag, s);
        if (int rc = scan_i32(ctx, ctx->sK1.as<int32_t>(), ctx->sV1.as<int32_t>(), (size_t)(3 * E) + 1)) return rc;
        int32_t h_pairs = 0;
        HIPCHK(hipMemcpyAsync(&h_pairs, ctx->sV1.as<int32_t>() + 3 * E, 4, hipMemcpyDeviceToHost, s));
        magk::incidence_emit(ctx->conn.as<int32_t>(), E, ctx->iperm.as<int32_t>(), N, ctx->sV1.as<int32_t>(),
                             ctx->sK0.as<uint32_t>(), ctx->sV0.as<uint32_t>(), counted ? nullptr : ctx->deg.as<int32_t>(), s);
        HIPCHK(hipStreamSynchronize(s));
        if (h_pairs > 0)
            if (int rc = sort_u32(ctx, ctx->sK0.as<uint32_t>(), ctx->sK1.as<uint32_t>(), ctx->sV0.as<uint32_t>(),
                                  ctx->inc.as<uint32_t>(), (size_t)h_pairs, ctx->bitsN))
                return rc;
    } else {
    magk::incidence_keys(ctx->conn.as<int32_t>(), E, ctx->iperm.as<int32_t>(), N, ctx->sK0.as<uint32_t>(),
                         ctx->sV0.as<uint32_t>(), counted ? nullptr : ctx->deg.as<int32_t>(), errflag, s);
    if (int rc = sort_u32(ctx, ctx->sK0.as<uint32_t>(), ctx->sK1.as<uint32_t>(), ctx->sV0.as<uint32_t>(),
                          ctx->inc.as<uint32_t>(), (size_t)(3 * E), ctx->bitsN))
        return rc;
    }
    if (int rc = scan_i32(ctx, ctx->deg.as<int32_t>(), ctx->inc_off.as<int32_t>(), (size_t)N + 1)) return rc;
    HIPCHK(hipMemsetAsync(ctx->tile_cnt.as<int64_t>() + T, 0, 8, s));
    magk::tile_degree(ctx->deg.as<int32_t>(), N, B, T, ctx->tile_deg.as<int32_t>(), ctx->tile_cnt.as<int64_t>(), s);
    if (int rc = scan_i64(ctx, ctx->tile_cnt.as<int64_t>(), ctx->tile_off.as<int64_t>(), (size_t)T + 1)) return rc;

    // tile-local numbering: references of every node to nodes of other tiles
    HIPCHK(ctx->hcnt.reserve(4 * ((size_t)N + 1)));
    HIPCHK(ctx->hoffn.reserve(4 * ((size_t)N + 1)));
    HIPCHK(ctx->tile_hcnt.reserve(4 * ((size_t)T + 1)));
    HIPCHK(ctx->tile_hoff.reserve(4 * ((size_t)T + 1)));
    magk::halo_count(ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(), ctx->conn.as<int32_t>(),
                     ctx->iperm.as<int32_t>(), N, B, ctx->hcnt.as<int32_t>(), s);
    if (int rc = scan_i32(ctx, ctx->hcnt.as<int32_t>(), ctx->hoffn.as<int32_t>(), (size_t)N + 1)) return rc;

    int32_t h_errk[2] = {0, 0}, h_refs = 0;
    int64_t h_total = 0;
    HIPCHK(hipMemcpyAsync(h_errk, errflag, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h_total, ctx->tile_off.as<int64_t>() + T, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h_refs, ctx->hoffn.as<int32_t>() + N, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_errk[0]) return fail(ctx, MAG_ERR_BAD_ARGS, "element node index out of range [0, %lld)", (long long)N);
    ctx->ell_total = h_total;
    ctx->nf = 2 * N - h_errk[1];
    if (ctx->nf == 0) return fail(ctx, MAG_ERR_BC_MISMATCH, "no unknown displacement in the boundary-condition set");

    HIPCHK(hipMemsetAsync(ctx->tile_hcnt.p, 0, 4 * ((size_t)T + 1), s));
    int32_t max_halo = 0;
    ctx->halo_total = 0;
    if (h_refs > 0) {
        const size_t nr = (size_t)h_refs;
        HIPCHK(ctx->hk0.reserve(8 * nr));
        HIPCHK(ctx->hk1.reserve(8 * nr));
        HIPCHK(ctx->head.reserve(4 * nr));
        HIPCHK(ctx->blk.reserve(4 * nr));
        HIPCHK(ctx->halo_g.reserve(4 * nr));
        magk::halo_emit(ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(), ctx->conn.as<int32_t>(),
                        ctx->iperm.as<int32_t>(), N, B, ctx->hoffn.as<int32_t>(), ctx->hk0.as<uint64_t>(), s);
        {
            size_t tb = 0;
            const int end_bit = 32 + ceil_log2(T);
            HIPCHK(magp::sort_keys_u64(nullptr, &tb, ctx->hk0.as<uint64_t>(), ctx->hk1.as<uint64_t>(), nr, 0, end_bit, s));
            if (int rc = scratch_for(ctx, tb)) return rc;
            HIPCHK(magp::sort_keys_u64(ctx->scratch.p, &tb, ctx->hk0.as<uint64_t>(), ctx->hk1.as<uint64_t>(), nr, 0,
                                       end_bit, s));
        }
        magk::csr_heads(ctx->hk1.as<uint64_t>(), (int64_t)nr, ctx->head.as<int32_t>(), s);
        if (int rc = scan_i32(ctx, ctx->head.as<int32_t>(), ctx->blk.as<int32_t>(), nr)) return rc;
        magk::halo_unique(ctx->hk1.as<uint64_t>(), ctx->head.as<int32_t>(), ctx->blk.as<int32_t>(), (int64_t)nr,
                          ctx->halo_g.as<int32_t>(), ctx->tile_hcnt.as<int32_t>(), s);
    } else {
        HIPCHK(ctx->halo_g.reserve(64));
    }
    if (int rc = scan_i32(ctx, ctx->tile_hcnt.as<int32_t>(), ctx->tile_hoff.as<int32_t>(), (size_t)T + 1)) return rc;
    {
        std::vector<int32_t> hc((size_t)T + 1);
        HIPCHK(hipMemcpyAsync(hc.data(), ctx->tile_hcnt.p, 4 * ((size_t)T + 1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int32_t t = 0; t < T; ++t) {
            if (hc[t] > max_halo) max_halo = hc[t];
            ctx->halo_total += hc[t];
        }
    }
    // ---- partition: contiguous tile ranges of the Hilbert order, identical arithmetic on every rank ----
    {
        ctx->own0 = (int32_t)std::min<int64_t>((int64_t)ctx->t0 * B, N);
        ctx->own1 = (int32_t)std::min<int64_t>((int64_t)ctx->t1 * B, N);
        ctx->dist = R > 1 || getenv("MAG_TUNE_FORCE_DIST") != nullptr;
        ctx->n_iface = 0;
        if (sh) {
            // the interface from one pass over the elements (symbolic.hip, k_iface_mark): the halo lists of the other ranks'
            // tiles are not there to derive it from
            // (marked by the pass that found the needed tiles; hcnt / hoffn: free since the halo references were emitted)
            magk::iface_flags(ctx->iface_mask.as<uint8_t>(), N, ctx->hcnt.as<int32_t>(), s);
            if (int rc = scan_i32(ctx, ctx->hcnt.as<int32_t>(), ctx->hoffn.as<int32_t>(), (size_t)N + 1)) return rc;
            int32_t h_ni = 0;
            HIPCHK(hipMemcpyAsync(&h_ni, ctx->hoffn.as<int32_t>() + N, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            ctx->n_iface = h_ni;
            HIPCHK(ctx->iface.reserve(4 * ((size_t)h_ni + 1)));
            HIPCHK(ctx->iface_readers.reserve((size_t)h_ni + 16));
            magk::iface_emit(ctx->iface_mask.as<uint8_t>(), ctx->hoffn.as<int32_t>(), N, ctx->iface.as<int32_t>(),
                             ctx->iface_readers.as<uint8_t>(), s);
        } else if (R > 1) {
            // interface = every node some rank reads (tile halo) but does not own; every rank derives the same
            // sorted list from the replicated symbolic data, so no communication is needed to agree on it
            std::vector<int32_t> hoff((size_t)T + 1), hg((size_t)std::max<int64_t>(ctx->halo_total, 1));
            HIPCHK(hipMemcpyAsync(hoff.data(), ctx->tile_hoff.p, 4 * ((size_t)T + 1), hipMemcpyDeviceToHost, s));
            if (ctx->halo_total > 0)
                HIPCHK(hipMemcpyAsync(hg.data(), ctx->halo_g.p, 4 * (size_t)ctx->halo_total, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            std::vector<int32_t> iface;
            std::vector<std::pair<int32_t, int32_t>> reads; // (node, reading rank)
            for (int r_ = 0; r_ < R; ++r_) {
                const int32_t ta = rank_tile_lo(T, R, r_), tb = rank_tile_lo(T, R, r_ + 1);
                const int64_t lo = std::min<int64_t>((int64_t)ta * B, N);
                const int64_t hi = std::min<int64_t>((int64_t)tb * B, N);
                for (int32_t t = ta; t < tb; ++t)
                    for (int32_t k = hoff[t]; k < hoff[t + 1]; ++k)
                        if (hg[k] < lo || hg[k] >= hi) {
                            iface.push_back(hg[k]);
                            reads.emplace_back(hg[k], r_);
                        }
            }
            std::sort(iface.begin(), iface.end());
            iface.erase(std::unique(iface.begin(), iface.end()), iface.end());
            ctx->n_iface = (int32_t)iface.size();
            // which ranks read each interface node (on-chip multi-GPU CG: its owner stores q into their inboxes)
            std::vector<uint8_t> readers(iface.size() + 1, 0);
            for (const auto &pr : reads) {
                const size_t slot = std::lower_bound(iface.begin(), iface.end(), pr.first) - iface.begin();
                readers[slot] |= (uint8_t)(1u << (pr.second & 7));
            }
            HIPCHK(ctx->iface.reserve(4 * (iface.size() + 1)));
            HIPCHK(ctx->iface_readers.reserve(iface.size() + 16));
            if (!iface.empty()) {
                HIPCHK(hipMemcpyAsync(ctx->iface.p, iface.data(), 4 * iface.size(), hipMemcpyHostToDevice, s));
                HIPCHK(hipMemcpyAsync(ctx->iface_readers.p, readers.data(), iface.size(), hipMemcpyHostToDevice, s));
            }
            HIPCHK(hipStreamSynchronize(s)); // the host vectors must outlive the copies
        }
        HIPCHK(ctx->comm_pq.reserve(128));
        HIPCHK(ctx->comm_rr.reserve(8 * (1 + 2 * (size_t)ctx->n_iface) + 64));
    }
    if (sh) {
        // what all ranks must decide alike hangs on the largest halo of ANY tile (the LDS layout, on-chip or streaming): every
        // rank puts the largest of the tiles it built into its own word of a vector, one sum-all-reduce, the maximum
        double hv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        hv[me] = (double)max_halo;
        if (int rc = allreduce_host(ctx, hv, 8)) return rc;
        for (int r_ = 0; r_ < R; ++r_) max_halo = std::max(max_halo, (int32_t)hv[r_]);
    }
    ctx->max_halo = max_halo;
    ctx->cap = ((B + max_halo + 31) / 32) * 32;
    ctx->use_lds = ctx->opt.op_variant != 1 && ctx->cap <= magk::kMaxLdsNodes;
    ctx->fused = ctx->use_lds && ctx->opt.cg_variant != 0; // the fused iteration needs the tile-local tables
    if (ctx->use_lds) {
        HIPCHK(ctx->halo_xy.reserve(16 * (size_t)std::max<int64_t>(ctx->halo_total, 1)));
        magk::halo_coords(ctx->halo_g.as<int32_t>(), ctx->xyP.as<double>(), ctx->halo_total, ctx->halo_xy.as<double>(), s);
        HIPCHK(ctx->ell.reserve(4 * (size_t)(h_total > 0 ? h_total : 1)));
        // the assembly's copy of the corner words (k_assemble_fan): only when K is assembled and the tile image (256 B of
        // accumulators per row node + 20 B per staged node) fits a CU's LDS
        const bool csr_wanted = wants_csr(ctx);
        const char *how_asm = getenv("MAG_TUNE_ASSEMBLY");
        ctx->asm_ctile = csr_wanted && !(how_asm && strcmp(how_asm, "ctile") != 0) && (B == 256 || B == 512) &&
                         ctx->cap <= 4096 && magk::assemble_ctiles_lds(B, ctx->cap) <= 64 * 1024;
        if (ctx->asm_ctile) HIPCHK(ctx->ell_asm.reserve(4 * (size_t)(h_total > 0 ? h_total : 1)));
        if (ctx->asm_ctile) HIPCHK(ctx->ell_pos.reserve(2 * (size_t)(h_total > 0 ? h_total : 1)));
        magk::fill_ell16(ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(), ctx->conn.as<int32_t>(),
                         ctx->iperm.as<int32_t>(), ctx->tile_deg.as<int32_t>(), ctx->tile_off.as<int64_t>(),
                         ctx->tile_hoff.as<int32_t>(), ctx->halo_g.as<int32_t>(), N, B, T, ctx->ell.as<uint32_t>(),
                         ctx->asm_ctile ? ctx->ell_asm.as<uint32_t>() : nullptr,
                         ctx->asm_ctile ? ctx->ell_pos.as<uint16_t>() : nullptr, s);
        HIPCHK(ctx->tile_rdeg.reserve(2 * 4 * ((size_t)T + 1)));
        HIPCHK(ctx->row_info.reserve((size_t)T * B + 64));
        magk::ring16(ctx->tile_deg.as<int32_t>(), ctx->tile_off.as<int64_t>(), B, T, ctx->ell.as<uint32_t>(),
                     ctx->tile_rdeg.as<int32_t>(), magk::persist_block_entries(), ctx->row_info.as<uint8_t>(), s);
        HIPCHK(ctx->tmeta.reserve(sizeof(magk::TileMeta) * (size_t)T));
        magk::tile_meta(ctx->tile_rdeg.as<int32_t>(), ctx->tile_rdeg.as<int32_t>() + T, ctx->tile_off.as<int64_t>(),
                        ctx->tile_hoff.as<int32_t>(), T,
                        ctx->tmeta.as<magk::TileMeta>(), s);
        magk::mark_published(ctx->halo_g.as<int32_t>(), ctx->halo_total, ctx->maskP.as<uint8_t>(), s);
        if (sh) { // the edge-block eligibility of the WHOLE mesh: k_ring16's flag word, OR-ed over the ranks
            int32_t ff = 3;
            HIPCHK(hipMemcpyAsync(&ff, ctx->tile_rdeg.as<int32_t>() + 2 * (size_t)T, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            double fv[2] = {(double)(ff & 1), (double)((ff >> 1) & 1)};
            if (int rc = allreduce_host(ctx, fv, 2)) return rc;
            ctx->fan_flags_global = (fv[0] > 0.0 ? 1 : 0) | (fv[1] > 0.0 ? 2 : 0);
        }
    } else {
        HIPCHK(ctx->ell.reserve(8 * (size_t)(h_total > 0 ? h_total : 1)));
        magk::fill_ell(ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(), ctx->conn.as<int32_t>(),
                       ctx->iperm.as<int32_t>(), ctx->tile_deg.as<int32_t>(), ctx->tile_off.as<int64_t>(), N, B, T,
                       ctx->ell.as<int2>(), s);
    }
    HIPCHK(hipGetLastError());
    // on-chip CG: every tile resident at once (one workgroup per CU, kPersistNpt * 512 / B tiles each).  With several
    // ranks the decision uses only quantities every rank computes identically (the largest tile count of a rank, the
    // global halo bound, the window size), so all ranks take the same path.
    ctx->persist = false;
    const bool mg = R > 1;
    const bool forced_dist = ctx->dist && !mg; // single-rank rehearsal of the distributed protocol: streaming kernels
    if (ctx->opt.cg_variant == 2 && ctx->use_lds && !forced_dist && !ctx->persist_failed && ctx->opt.precision == 0 &&
        ctx->opt.preconditioner == 0 && ctx->opt.cg_operator == MAG_OP_MATRIX_FREE &&
        // the granule tags count the iterations: 32 bits on one GPU, 24 bits next to the solve sequence across GPUs
        ctx->opt.max_iter < (mg ? (int64_t(1) << 24) - 4 : (int64_t(1) << 31) - 4) &&
        (!mg || R > 8 ||
         ((ctx->inbox_ready ? ctx->inbox_bytes : (ctx->win_dev ? ctx->win_bytes : 0)) >=
          64 + 128 * (size_t)R + 64 * (size_t)ctx->n_iface)) && R <= 8) {
        int dev = 0, cus = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const int kmax = magk::persist_tiles_per_wg(B);
        const int32_t tiles_max = most_rank_tiles(T, R);
        int k = cus > 0 ? (tiles_max + cus - 1) / cus : 0;
        // a mesh of at most kmax tiles on one GPU (up to 2048 nodes: the size of the reference's own examples) goes to ONE
        // workgroup: every tile is a sibling of every other, nothing is exchanged through memory (persist_single_workgroup)
        if (!mg && tiles_max <= kmax) k = std::max(k, (int)tiles_max);
        // rehearsals: several ranks share ONE GPU and must all be co-resident -- fewer, fuller workgroups per rank
        k = std::max(k, env_int("MAG_TUNE_PERSIST_K", 0));
        // Measured against the streaming kernel on the same 512-node tiles the on-chip kernel wins from one tile per
        // workgroup up (6.2 vs 7.9 us per iteration at 115 tiles, 12.6 vs 20.3 at 982); with 256-node tiles it does not
        // (and eight of them rarely fit the LDS), so those only run it when a test asks (MAG_TUNE_PERSIST_MIN_K=1).
        const int kmin = env_int("MAG_TUNE_PERSIST_MIN_K", B == 512 ? 1 : 9);
        ctx->persist_maxh = ((max_halo + 3) / 4) * 4;
        if (kmax > 0 && k >= 1 && k >= kmin && k <= kmax && (tiles_max + k - 1) / k <= 256 && // the gather holds 256
            (int64_t)k * max_halo <= 2 * 512 && // a workgroup's halo entries are dealt out two per thread (of 512)
            magk::persist_lds_bytes(B, ctx->cap, ctx->persist_maxh, 0, 0, mg) + 256 <= 160 * 1024 && // + the static 256 bytes
            (!mg || ctx->n_iface < (1 << 24))) { // (interface slots are kept in 24 bits on the chip)
            ctx->persist = true;
            ctx->persist_k = k;
            ctx->persist_grid = (ctx->t1 - ctx->t0 + k - 1) / k;
        }
    }
    ctx->have_order = true;
    return MAG_OK;
}

// ---- symbolic phase 2 + numeric assembly: K in CSR, caller numbering ----
int csr_symbolic(mag_ctx *ctx)
{
    ctx->bc_touch_ready = false;
    ctx->fc_ready = false; // (... and of this pattern's block numbering)
    const int64_t N = ctx->N, E = ctx->E;
    int64_t n9 = 9 * E;
    hipStream_t s = ctx->stream;
    // Several ranks: each keeps the rows of its own nodes, of its tiles' halo nodes (one ghost layer: the ghost
    // recurrences need their right-hand side) and of the prescribed nodes (reactions on every rank, no second
    // collective): solver.rs:304-322 couples rows only through shared elements, so those rows are complete.  Rows a
    // rank does not keep get no blocks, so the pattern, K and every pass over them shrink with the rank count.
    const bool shard = ctx->comm.nranks > 1 && !ctx->want_full_csr;
    ctx->csr_full = !shard;
    if (shard) {
        HIPCHK(ctx->local_node.reserve((size_t)N + 64));
        HIPCHK(hipMemsetAsync(ctx->local_node.p, 0, (size_t)N, s));
        std::vector<int32_t> h2(2);
        HIPCHK(hipMemcpyAsync(&h2[0], ctx->tile_hoff.as<int32_t>() + ctx->t0, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&h2[1], ctx->tile_hoff.as<int32_t>() + ctx->t1, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        magk::mark_local(ctx->perm.as<uint32_t>(), ctx->maskP.as<uint8_t>(), N, ctx->own0, ctx->own1,
                         ctx->halo_g.as<int32_t>(), h2[0], h2[1], ctx->local_node.as<uint8_t>(), s);
    }
    HIPCHK(ctx->rowcnt.reserve(4 * ((size_t)N + 1)));
    HIPCHK(ctx->bptr.reserve(4 * ((size_t)N + 1)));
    // Default: the pattern straight from the incidence lists (k_pattern_rows: no pair list, no 9E-key sort -- 0.15 ms
    // instead of 0.9 ms at 1M triangles).  The sort-based pattern below serves rows too long for its register array
    // (valence >= 16); MAG_TUNE_PATTERN_SORT=1 takes it for every mesh.
    if (!getenv("MAG_TUNE_PATTERN_SORT")) {
        int32_t *ovf = (int32_t *)(ctx->small.as<double>() + 4 * 256 + 4) + 2;
        const uint8_t *local = shard ? ctx->local_node.as<uint8_t>() : nullptr;
        HIPCHK(hipMemsetAsync(ovf, 0, 4, s));
        const uint8_t *need = shard && ctx->order_sharded ? ctx->need_tile.as<uint8_t>() : nullptr;
        magk::pattern_count(ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(), ctx->perm.as<uint32_t>(),
                            ctx->conn.as<int32_t>(), local, N, ctx->rowcnt.as<int32_t>(), ovf, need, ctx->B, s);
        if (int rc = scan_i32(ctx, ctx->rowcnt.as<int32_t>(), ctx->bptr.as<int32_t>(), (size_t)N + 1)) return rc;
        int32_t h_nb = 0, h_ovf = 0;
        HIPCHK(hipMemcpyAsync(&h_nb, ctx->bptr.as<int32_t>() + N, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&h_ovf, ovf, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!h_ovf) {
            const int64_t nb = h_nb;
            if (nb <= 0) return fail(ctx, MAG_ERR_STATE, "rank %d keeps no row of K", ctx->comm.rank);
            if (4 * nb >= (int64_t(1) << 31))
                return fail(ctx, MAG_ERR_TOO_LARGE, "nnz of K (%lld) exceeds int32", (long long)(4 * nb));
            ctx->nb = nb;
            HIPCHK(ctx->bcol.reserve(4 * (size_t)nb));
            HIPCHK(ctx->kval.reserve(8 * 4 * (size_t)nb));
            HIPCHK(ctx->bc_touch.reserve((size_t)N + 16));
            magk::pattern_fill(ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(), ctx->perm.as<uint32_t>(),
                               ctx->conn.as<int32_t>(), local, N, ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(),
                               ctx->uknown.as<uint8_t>(), ctx->bc_touch.as<uint8_t>(), need, ctx->B, s);
            ctx->bc_touch_ready = true;
            HIPCHK(hipGetLastError());
            return MAG_OK;
        }
    }
    if (shard) {
        HIPCHK(ctx->ecnt.reserve(4 * ((size_t)E + 1)));
        HIPCHK(ctx->eoff.reserve(4 * ((size_t)E + 1)));
        magk::csr_pair_count(ctx->conn.as<int32_t>(), E, ctx->local_node.as<uint8_t>(), ctx->ecnt.as<int32_t>(), s);
        if (int rc = scan_i32(ctx, ctx->ecnt.as<int32_t>(), ctx->eoff.as<int32_t>(), (size_t)E + 1)) return rc;
        int32_t h_n = 0;
        HIPCHK(hipMemcpyAsync(&h_n, ctx->eoff.as<int32_t>() + E, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        n9 = h_n;
        if (n9 <= 0) return fail(ctx, MAG_ERR_STATE, "rank %d keeps no row of K", ctx->comm.rank);
    }
    HIPCHK(ctx->pk0.reserve(8 * (size_t)n9));
    HIPCHK(ctx->pk1.reserve(8 * (size_t)n9));
    HIPCHK(ctx->pv0.reserve(4 * (size_t)n9));
    HIPCHK(ctx->pv1.reserve(4 * (size_t)n9));
    HIPCHK(ctx->head.reserve(4 * (size_t)n9));
    HIPCHK(ctx->blk.reserve(4 * (size_t)n9));
    HIPCHK(ctx->rowcnt.reserve(4 * ((size_t)N + 1)));
    HIPCHK(ctx->bptr.reserve(4 * ((size_t)N + 1)));
    if (shard)
        magk::csr_pairs_local(ctx->conn.as<int32_t>(), E, ctx->local_node.as<uint8_t>(), ctx->eoff.as<int32_t>(),
                              ctx->pk0.as<uint64_t>(), ctx->pv0.as<uint32_t>(), s);
    else
        magk::csr_pairs(ctx->conn.as<int32_t>(), E, ctx->pk0.as<uint64_t>(), ctx->pv0.as<uint32_t>(), s);
    if (int rc = sort_u64(ctx, ctx->pk0.as<uint64_t>(), ctx->pk1.as<uint64_t>(), ctx->pv0.as<uint32_t>(),
                          ctx->pv1.as<uint32_t>(), (size_t)n9, 32 + ctx->bitsN))
        return rc;
    magk::csr_heads(ctx->pk1.as<uint64_t>(), n9, ctx->head.as<int32_t>(), s);
    if (int rc = scan_i32(ctx, ctx->head.as<int32_t>(), ctx->blk.as<int32_t>(), (size_t)n9)) return rc;
    int32_t h_last[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&h_last[0], ctx->blk.as<int32_t>() + (n9 - 1), 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h_last[1], ctx->head.as<int32_t>() + (n9 - 1), 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int64_t nb = (int64_t)h_last[0] + h_last[1];
    if (4 * nb >= (int64_t(1) << 31))
        return fail(ctx, MAG_ERR_TOO_LARGE, "nnz of K (%lld) exceeds int32", (long long)(4 * nb));
    ctx->nb = nb;
    HIPCHK(ctx->seg_start.reserve(4 * ((size_t)nb + 1)));
    HIPCHK(ctx->brow.reserve(4 * (size_t)nb));
    HIPCHK(ctx->bcol.reserve(4 * (size_t)nb));
    HIPCHK(ctx->kval.reserve(8 * 4 * (size_t)nb));
    HIPCHK(hipMemsetAsync(ctx->rowcnt.p, 0, 4 * ((size_t)N + 1), s));
    magk::csr_segments(ctx->pk1.as<uint64_t>(), ctx->head.as<int32_t>(), ctx->blk.as<int32_t>(), n9,
                       ctx->seg_start.as<int32_t>(), ctx->brow.as<int32_t>(), ctx->bcol.as<int32_t>(),
                       ctx->rowcnt.as<int32_t>(), s);
    if (int rc = scan_i32(ctx, ctx->rowcnt.as<int32_t>(), ctx->bptr.as<int32_t>(), (size_t)N + 1)) return rc;
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

int element_phase(mag_ctx *ctx)
{
    HIPCHK(ctx->ke.reserve(8 * 36 * (size_t)ctx->E));
    magk::element_stiffness(ctx->xy.as<double>(), ctx->conn.as<int32_t>(), ctx->E, ctx->nu, ctx->youngs, ctx->thick,
                            ctx->ke.as<double>(), ctx->stream);
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

// numeric assembly, atomic-free, K_e evaluated on the fly (no 288-byte-per-element buffer): from the CG tiles
// (k_assemble_fan) where their image fits, otherwise per element tile with LDS staging (k_assemble_tiles).  Bit-identical.
bool assemble_from_ctiles(const mag_ctx *ctx)
{
    const char *how = getenv("MAG_TUNE_ASSEMBLY");
    return ctx->asm_ctile && ctx->use_lds && !(how && !strcmp(how, "tiles"));
}

// ---- mag_options.field_cg: the block-row table of K, once per order and pattern; the gathered values, once per assembly ----
// The table of the order and the pattern held now, in the buffers of its owner: a field's (fc_*, ensure_field_table) or the
// passes' on the assembled pattern (ptab, pass_table).  val: room for the gathered values
struct FieldTable {
    DevBuf &width, &meta, &slot, &src, &val;
    int64_t total = 0;
};

inline FieldTable pass_table(mag_ctx *ctx) { return {ctx->ptab.width, ctx->ptab.meta, ctx->ptab.slot, ctx->ptab.src, ctx->ptab.val}; }

int build_field_table(mag_ctx *ctx, FieldTable &tab)
{
    using magk::FieldTileMeta;
    hipStream_t s = ctx->stream;
    const int32_t T = ctx->T, B = ctx->B;
    HIPCHK(tab.width.reserve(4 * (size_t)T + 64));
    magk::field_widths(ctx->bptr.as<int32_t>(), ctx->perm.as<uint32_t>(), ctx->N, B, T, tab.width.as<int32_t>(), s);
    std::vector<int32_t> width((size_t)T), hoff((size_t)T + 1);
    HIPCHK(hipMemcpyAsync(width.data(), tab.width.p, 4 * (size_t)T, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hoff.data(), ctx->tile_hoff.p, 4 * ((size_t)T + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<FieldTileMeta> meta((size_t)T);
    int64_t total = 0;
    for (int32_t t = 0; t < T; ++t) {
        meta[(size_t)t] = FieldTileMeta{total, width[(size_t)t], hoff[(size_t)t], hoff[(size_t)t + 1] - hoff[(size_t)t], 0, 0};
        total += (int64_t)width[(size_t)t] * B;
    }
    tab.total = total;
    HIPCHK(tab.meta.reserve(sizeof(FieldTileMeta) * (size_t)T));
    HIPCHK(tab.slot.reserve(2 * (size_t)total + 64));
    HIPCHK(tab.src.reserve(4 * (size_t)total + 64));
    HIPCHK(tab.val.reserve(2 * 16 * (size_t)total));
    HIPCHK(hipMemcpyAsync(tab.meta.p, meta.data(), sizeof(FieldTileMeta) * (size_t)T, hipMemcpyHostToDevice, s));
    int32_t *err = tab.width.as<int32_t>() + T; // (the spare words behind the widths)
    HIPCHK(hipMemsetAsync(err, 0, 4, s));
    magk::field_rows(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), ctx->perm.as<uint32_t>(), ctx->iperm.as<int32_t>(),
                     ctx->halo_g.as<int32_t>(), tab.meta.as<FieldTileMeta>(), ctx->N, B, T, tab.slot.as<uint16_t>(),
                     tab.src.as<int32_t>(), err, s);
    int32_t h_err = 0;
    HIPCHK(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s)); // (the host vectors must outlive the copies)
    if (h_err) return fail(ctx, MAG_ERR_STATE, "field_cg: a column of K is in neither its tile nor the tile's halo list");
    return MAG_OK;
}

// The numeric part for the matrix values `val` (kval's layout) on a table: the gathered copy with the Dirichlet mask applied
// and, for kind 1 | 2, the preconditioner's inverse node blocks (diagonal | 2 x 2) with their halo copies
int field_values(mag_ctx *ctx, const FieldTable &tab, const double *val, int kind, DevBuf &minv, DevBuf &hminv)
{
    using magk::FieldTileMeta;
    hipStream_t s = ctx->stream;
    magk::field_gather(ctx->bptr.as<int32_t>(), ctx->perm.as<uint32_t>(), val, ctx->maskP.as<uint8_t>(),
                       ctx->halo_g.as<int32_t>(), tab.meta.as<FieldTileMeta>(), tab.slot.as<uint16_t>(),
                       tab.src.as<int32_t>(), ctx->N, ctx->B, ctx->T, tab.total, tab.val.as<double2>(), s);
    if (kind) {
        HIPCHK(minv.reserve(16 * (size_t)ctx->N));
        HIPCHK(hminv.reserve(16 * (size_t)std::max<int64_t>(ctx->halo_total, 1)));
        magk::field_minv(ctx->bptr.as<int32_t>(), ctx->perm.as<uint32_t>(), val, ctx->maskP.as<uint8_t>(),
                         tab.meta.as<FieldTileMeta>(), tab.src.as<int32_t>(), ctx->N, ctx->B, kind, minv.as<float4>(), s);
        magk::halo_minv(ctx->halo_g.as<int32_t>(), minv.as<float4>(), ctx->halo_total, hminv.as<float4>(), s);
    }
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

int ensure_field_table(mag_ctx *ctx)
{
    if (ctx->fc_ready || !field_cg_selected(ctx)) return MAG_OK;
    const auto t_start = std::chrono::steady_clock::now();
    FieldTable tab{ctx->fc_width, ctx->fc_meta, ctx->fc_slot, ctx->fc_src, ctx->fc_val};
    if (int rc = build_field_table(ctx, tab)) return rc;
    ctx->fc_total = tab.total;
    ctx->fc_grid = magk::field_cg_grid(ctx->B, ctx->cap, ctx->T, ctx->opt.field_cg >= 2);
    ctx->fc_ready = true;
    ctx->fc_build_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return MAG_OK;
}

// after kval is written: the gathered copy with the Dirichlet mask applied, and the preconditioner's inverse node blocks
int field_numeric(mag_ctx *ctx)
{
    if (!field_cg_selected(ctx)) return MAG_OK;
    if (int rc = ensure_field_table(ctx)) return rc;
    FieldTable tab{ctx->fc_width, ctx->fc_meta, ctx->fc_slot, ctx->fc_src, ctx->fc_val, ctx->fc_total};
    const int kind = ctx->opt.field_cg >= 2 ? (ctx->opt.field_cg == 3 ? 2 : 1) : 0;
    return field_values(ctx, tab, ctx->kval.as<double>(), kind, ctx->minvP, ctx->halo_minv);
}

int assemble_values(mag_ctx *ctx)
{
    if (assemble_from_ctiles(ctx) &&
               magk::assemble_ctiles(ctx->bcol.as<int32_t>(), ctx->bptr.as<int32_t>(), ctx->perm.as<uint32_t>(),
                                     ctx->xyP.as<double>(), ctx->halo_xy.as<double>(),
                                     ctx->tile_hoff.as<int32_t>(), ctx->tile_deg.as<int32_t>(), ctx->tile_off.as<int64_t>(),
                                     ctx->ell_asm.as<uint32_t>(), ctx->ell_pos.as<uint16_t>(),
                                     ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(),
                                     ctx->conn.as<int32_t>(), ctx->xy.as<double>(), ctx->N, ctx->B, ctx->T, ctx->cap,
                                     ctx->nu, ctx->youngs, ctx->thick, ctx->kval.as<double>(), field_of(ctx), ctx->stream)) {
        // assembled from the CG tiles (coordinates and caller ids staged in LDS)
    } else {
        magk::assemble_tiles(ctx->bcol.as<int32_t>(), ctx->bptr.as<int32_t>(), ctx->inc_off.as<int32_t>(),
                             ctx->inc.as<uint32_t>(), ctx->perm.as<uint32_t>(), ctx->conn.as<int32_t>(),
                             ctx->xy.as<double>(), ctx->N, ctx->nu, ctx->youngs, ctx->thick, ctx->kval.as<double>(),
                             field_of(ctx), ctx->stream);
    }
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

int gather_phase(mag_ctx *ctx)
{
    if (int rc = assemble_values(ctx)) return rc;
    return field_numeric(ctx);
}

// K values of the variants of `vbat` (coordinates `xy`, permuted in v_xyP / v_halo) in the shared pattern, into v_kval:
// gather_phase's choice of kernel
void assemble_variant_values(mag_ctx *ctx, const double *xy, const magk::VariantBatch &vbat, hipStream_t s)
{
    if (assemble_from_ctiles(ctx) &&
        magk::assemble_ctiles_variants(ctx->bcol.as<int32_t>(), ctx->bptr.as<int32_t>(), ctx->perm.as<uint32_t>(),
                                       ctx->v_xyP.as<double>(), ctx->v_halo.as<double>(), ctx->tile_hoff.as<int32_t>(),
                                       ctx->tile_deg.as<int32_t>(), ctx->tile_off.as<int64_t>(), ctx->ell_asm.as<uint32_t>(),
                                       ctx->ell_pos.as<uint16_t>(), ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(),
                                       ctx->conn.as<int32_t>(), xy, ctx->N, ctx->B, ctx->T, ctx->cap, vbat, ctx->v_kval.as<double>(), s))
        return;
    magk::assemble_tiles_variants(ctx->bcol.as<int32_t>(), ctx->bptr.as<int32_t>(), ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(),
                                  ctx->perm.as<uint32_t>(), ctx->conn.as<int32_t>(), xy, ctx->N, vbat, ctx->v_kval.as<double>(), s);
}

// the whole mesh's tables: a run across ranks has left those of the tiles this rank needs only (order_sharded); the entry
// points that walk the whole mesh on ONE rank (all of K, plain operator applications) rebuild them here -- without the sharded
// phase's all-reduces, which only mag_run may enter
int ensure_full_order(mag_ctx *ctx)
{
    if (ctx->have_order && ctx->order_sharded) ctx->have_order = ctx->have_csr = false;
    return ensure_order(ctx);
}

// all of K, for the entry points that hand K out (mag_assemble_csr, mag_reduce_system): a multi-rank context whose run
// kept only its own rows builds the whole matrix here
int ensure_csr(mag_ctx *ctx)
{
    if (ctx->have_csr && ctx->csr_full) return MAG_OK;
    FieldOperator op(ctx);
    if (int rc = ensure_full_order(ctx)) return rc; // validates conn
    int rc = MAG_OK;
    if (!(ctx->field_on && ctx->field_sym)) { // (under a field the pattern of its first run stays)
        ctx->want_full_csr = true;
        rc = csr_symbolic(ctx);
        ctx->want_full_csr = false;
        if (rc) return rc;
        ctx->field_sym = ctx->field_on;
    }
    if ((rc = gather_phase(ctx))) return rc;
    ctx->have_csr = true;
    return MAG_OK;
}

magk::OpParams op_params(mag_ctx *ctx)
{
    magk::OpParams P = {};
    P.N = ctx->N;
    P.T = ctx->T;
    P.t0 = 0; // plain applications (RHS, reactions, tests) always cover the whole mesh
    P.t1 = ctx->T;
    P.own0 = 0;
    P.own1 = (int32_t)ctx->N;
    P.nPart = magk::cg_grid(ctx->T);
    P.xyP = ctx->xyP.as<double2>();
    P.maskP = ctx->maskP.as<uint8_t>();
    P.tile_deg = (ctx->use_lds ? ctx->tile_rdeg : ctx->tile_deg).as<int32_t>(); // LDS tables are in ring form
    P.tile_off = ctx->tile_off.as<int64_t>();
    if (ctx->use_lds) {
        P.ell16 = ctx->ell.as<uint32_t>();
        P.tile_hoff = ctx->tile_hoff.as<int32_t>();
        P.halo_g = ctx->halo_g.as<int32_t>();
        P.halo_xy = ctx->halo_xy.as<double2>();
        P.cap = ctx->cap;
    } else {
        P.ell = ctx->ell.as<int2>();
    }
    P.wt = 1; // write-through (sc1) stores of p, q, x, r
    set_material(ctx, P);
    return P;
}

int apply_plain(mag_ctx *ctx, const double *vP, double *yP, int masked, bool owned_only = false)
{
    magk::OpParams P = op_params(ctx);
    if (owned_only) { // timing helper at N > 1: only the tiles this rank owns
        P.t0 = ctx->t0;
        P.t1 = ctx->t1;
        P.own0 = ctx->own0;
        P.own1 = ctx->own1;
    }
    P.v = (const double2 *)vP;
    P.y = (double2 *)yP;
    P.masked = masked;
    magk::op_launch(P, ctx->B, false, ctx->stream);
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

int reserve_cg(mag_ctx *ctx)
{
    const size_t vb = 16 * (size_t)ctx->N;
    HIPCHK(ctx->x.reserve(vb));
    HIPCHK(ctx->r.reserve(vb));
    HIPCHK(ctx->p0.reserve(vb));
    HIPCHK(ctx->p1.reserve(vb));
    HIPCHK(ctx->q.reserve(vb));
    HIPCHK(ctx->bP.reserve(vb));
    HIPCHK(ctx->tmpP.reserve(vb));
    HIPCHK(ctx->partRR.reserve(8 * magk::kMaxGrid));
    HIPCHK(ctx->partPQ.reserve(8 * magk::kMaxGrid));
    HIPCHK(ctx->state.reserve(sizeof(CgState)));
    HIPCHK(ctx->hist.reserve(8 * (size_t)(ctx->opt.history_len > 0 ? ctx->opt.history_len : 1)));
    return MAG_OK;
}

void iteration_params(mag_ctx *ctx, int parity, magk::OpParams &P, magk::UpdParams &U)
{
    P = op_params(ctx);
    P.t0 = ctx->t0;
    P.t1 = ctx->t1;
    P.own0 = ctx->own0;
    P.own1 = ctx->own1;
    P.iface = ctx->iface.as<int32_t>();
    P.n_iface = ctx->n_iface;
    P.nPart = ctx->dist ? 1 : magk::cg_grid(ctx->t1 - ctx->t0);
    P.r = ctx->r.as<double2>();
    P.pprev = parity ? ctx->p0.as<double2>() : ctx->p1.as<double2>();
    P.pnew = parity ? ctx->p1.as<double2>() : ctx->p0.as<double2>();
    P.q = ctx->q.as<double2>();
    P.x = ctx->x.as<double2>();
    // distributed: the dots arrive all-reduced in comm_rr[0] / comm_pq[0]; kernels still write local partials
    P.partRR = ctx->dist ? ctx->comm_rr.as<double>() : ctx->partRR.as<double>();
    P.partPQ = ctx->partPQ.as<double>();
    P.st = ctx->state.as<CgState>();
    P.hist = ctx->hist.as<double>();
    P.hist_len = ctx->opt.history_len;
    U = {};
    U.N = ctx->N;
    U.T = ctx->T;
    U.nPart = P.nPart;
    U.t0 = ctx->t0;
    U.t1 = ctx->t1;
    U.r = ctx->r.as<double2>();
    U.q = ctx->q.as<double2>();
    U.partPQ = ctx->dist ? ctx->comm_pq.as<double>() : ctx->partPQ.as<double>();
    U.partRR = ctx->partRR.as<double>();
    U.st = ctx->state.as<CgState>();
    U.wt = 1; // write-through stores
}

// one block of G CG iterations on the stream (parity 0 first: p_prev = p1, p_new = p0)
int launch_block(mag_ctx *ctx, int G)
{
    const int nloc = magk::cg_grid(ctx->t1 - ctx->t0);
    for (int i = 0; i < G; ++i) {
        magk::OpParams P;
        magk::UpdParams U;
        iteration_params(ctx, i & 1, P, U);
        magk::op_launch(P, ctx->B, true, ctx->stream);
        if (ctx->dist) {
            // p.q: sum of this rank's partials -> comm_pq[0] -> sum over ranks
            magk::iface_pack(ctx->partPQ.as<double>(), nloc, nullptr, nullptr, 0, 0, 0, ctx->comm_pq.as<double>(),
                             ctx->stream);
            if (int rc = allreduce(ctx, ctx->comm_pq.as<double>(), 1)) return rc;
        }
        magk::upd_launch(U, ctx->B, ctx->stream);
        if (ctx->dist) {
            // one buffer: [r.r partial sum | r on the interface nodes this rank owns], summed over ranks,
            // then the other ranks' interface residuals are written into this rank's copy of r
            magk::iface_pack(ctx->partRR.as<double>(), nloc, ctx->r.as<double2>(), ctx->iface.as<int32_t>(),
                             ctx->n_iface, ctx->own0, ctx->own1, ctx->comm_rr.as<double>(), ctx->stream);
            if (int rc = allreduce(ctx, ctx->comm_rr.as<double>(), 1 + 2 * (int64_t)ctx->n_iface)) return rc;
            magk::iface_unpack(ctx->comm_rr.as<double>(), ctx->iface.as<int32_t>(), ctx->n_iface, ctx->own0,
                               ctx->own1, ctx->r.as<double2>(), ctx->stream);
        }
    }
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

// the fields every graph key holds: the buffers and scalars the captured launches read (at most 18 words), the sizes, and
// the material constants, which are baked into the kernel arguments too
mag_ctx::GraphKey graph_key(const mag_ctx *ctx, int G, std::initializer_list<void *> ptrs)
{
    mag_ctx::GraphKey k = {};
    assert(ptrs.size() <= 18);
    std::copy(ptrs.begin(), ptrs.end(), k.ptrs);
    k.N = ctx->N;
    k.T = ctx->T;
    k.B = ctx->B;
    k.G = G;
    k.hist_len = ctx->opt.history_len;
    const double mat[2] = {ctx->youngs * ctx->thick, ctx->nu};
    memcpy(&k.ptrs[18], mat, sizeof mat);
    return k;
}

// ctx->graph: the block `enqueue` puts on the stream, captured again whenever the key differs from the last one
template <class Enqueue>
int capture_graph(mag_ctx *ctx, const mag_ctx::GraphKey &k, Enqueue enqueue)
{
    if (ctx->graph && memcmp(&k, &ctx->gkey, sizeof k) == 0) return MAG_OK;
    if (ctx->graph) {
        (void)hipGraphExecDestroy(ctx->graph);
        ctx->graph = nullptr;
    }
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, MAG_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(&ctx->graph, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
        ctx->graph = nullptr;
        return fail(ctx, MAG_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ei));
    }
    ctx->gkey = k;
    return MAG_OK;
}

int ensure_graph(mag_ctx *ctx, int G)
{
    const mag_ctx::GraphKey k =
        graph_key(ctx, G, {ctx->x.p, ctx->r.p, ctx->p0.p, ctx->p1.p, ctx->q.p, ctx->partRR.p, ctx->partPQ.p, ctx->state.p,
                           ctx->hist.p, ctx->xyP.p, ctx->maskP.p, ctx->tile_deg.p, ctx->tile_off.p, ctx->ell.p,
                           ctx->tile_hoff.p, ctx->halo_g.p, (void *)(intptr_t)(ctx->use_lds ? ctx->cap : -1), ctx->halo_xy.p});
    return capture_graph(ctx, k, [&] { return launch_block(ctx, G); });
}

int launch_graph(mag_ctx *ctx)
{
    HIPCHK(hipGraphLaunch(ctx->graph, ctx->stream));
    return MAG_OK;
}

// solver.rs:139-176's loop, G iterations per block (enqueue_block): the host polls the device-side state one block behind
// the one it has just queued, so the GPU never waits for the host.  Iterate j is produced by launch j and judged by launch
// j+1: up to two launches more than iterations.
template <class State, class Enqueue>
int run_blocks(mag_ctx *ctx, const DevBuf &dev_state, State *host_slots, Enqueue enqueue_block)
{
    hipStream_t s = ctx->stream;
    const long long max_blocks = (long long)(ctx->opt.max_iter / ctx->opt.check_every) + 3;
    bool done = false;
    int slot = 0;
    for (long long blk = 0; blk < max_blocks && !done; ++blk) {
        if (int rc = enqueue_block()) return rc;
        HIPCHK(hipMemcpyAsync(&host_slots[slot], dev_state.p, sizeof(State), hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(ctx->evPoll[slot], s));
        if (blk >= 1) {
            HIPCHK(hipEventSynchronize(ctx->evPoll[slot ^ 1]));
            done = host_slots[slot ^ 1].done != 0;
        }
        slot ^= 1;
    }
    return MAG_OK;
}

// the final state of a solve (CgState or FusedState) into the statistics and argmin's best_param bookkeeping
template <class State>
void take_stats(mag_ctx *ctx, const State &st)
{
    ctx->stats.iterations = st.iterations;
    ctx->stats.final_cost = st.final_cost;
    ctx->stats.rhs_norm = std::sqrt(st.bb);
    ctx->stats.converged = st.converged;
    ctx->stats.breakdown = st.breakdown;
    ctx->best_cost = st.best_cost;
    ctx->best_iter = st.best_iter;
}

// Every rank returns the whole solution, as solver::run would: the owned node ranges (contiguous in the Hilbert order,
// equal up to one tile) are all-gathered -- (R-1)/R of the vector per GPU over the ring, half of what summing a
// zero-padded full vector costs -- and copied to their places.
int gather_solution(mag_ctx *ctx)
{
    const int R = ctx->comm.nranks;
    if (R <= 1 && !ctx->dist) return MAG_OK;
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N, B = ctx->B, T = ctx->T;
    auto lo = [&](int r) { return std::min<int64_t>(rank_tile_lo(T, R, r) * B, N); };
    int64_t most = 0;
    for (int r = 0; r < R; ++r) most = std::max(most, lo(r + 1) - lo(r));
    const size_t cnt = 2 * (size_t)most; // doubles per rank
    HIPCHK(ctx->gath_send.reserve(8 * cnt + 64));
    HIPCHK(ctx->gath_recv.reserve(8 * cnt * (size_t)R + 64));
    const int64_t mine = ctx->own1 - ctx->own0;
    HIPCHK(hipMemsetAsync(ctx->gath_send.p, 0, 8 * cnt, s));
    HIPCHK(hipMemcpyAsync(ctx->gath_send.p, ctx->x.as<double>() + 2 * (size_t)ctx->own0, 16 * (size_t)mine,
                          hipMemcpyDeviceToDevice, s));
    if (int rc = allgather(ctx, ctx->gath_send.as<double>(), ctx->gath_recv.as<double>(), (int64_t)cnt)) return rc;
    for (int r = 0; r < R; ++r)
        if (lo(r + 1) > lo(r))
            HIPCHK(hipMemcpyAsync(ctx->x.as<double>() + 2 * (size_t)lo(r), ctx->gath_recv.as<double>() + cnt * (size_t)r,
                                  16 * (size_t)(lo(r + 1) - lo(r)), hipMemcpyDeviceToDevice, s));
    return MAG_OK;
}

// solver.rs:139-176 on the device: two launches per iteration (operator, update)
int cg_phase(mag_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const size_t vb = 16 * (size_t)ctx->N;
    HIPCHK(hipMemsetAsync(ctx->x.p, 0, vb, s));
    HIPCHK(hipMemsetAsync(ctx->p0.p, 0, vb, s));
    HIPCHK(hipMemsetAsync(ctx->p1.p, 0, vb, s));
    magk::cg_init(ctx->bP.as<double2>(), ctx->r.as<double2>(), ctx->N, ctx->B, ctx->T, ctx->t0, ctx->t1,
                  ctx->partRR.as<double>(), s);
    if (ctx->dist) {
        magk::iface_pack(ctx->partRR.as<double>(), magk::cg_grid(ctx->T), nullptr, nullptr, 0, 0, 0,
                         ctx->comm_rr.as<double>(), s);
        if (int rc = allreduce(ctx, ctx->comm_rr.as<double>(), 1)) return rc;
        magk::cg_setup(ctx->comm_rr.as<double>(), 1, ctx->opt.stop_mode, ctx->opt.tol, (long long)ctx->opt.max_iter,
                       ctx->state.as<CgState>(), s);
    } else {
        magk::cg_setup(ctx->partRR.as<double>(), magk::cg_grid(ctx->T), ctx->opt.stop_mode, ctx->opt.tol,
                       (long long)ctx->opt.max_iter, ctx->state.as<CgState>(), s);
    }
    HIPCHK(hipGetLastError());

    const int G = ctx->opt.check_every;
    // the distributed block carries collectives (and, with the test transport, host round trips): launched eagerly
    const bool graph = ctx->opt.use_graph != 0 && !ctx->dist;
    if (graph)
        if (int rc = ensure_graph(ctx, G)) return rc;
    if (int rc = run_blocks(ctx, ctx->state, ctx->h_state, [&] { return graph ? launch_graph(ctx) : launch_block(ctx, G); }))
        return rc;
    if (ctx->dist)
        if (int rc = gather_solution(ctx)) return rc;
    HIPCHK(hipMemcpyAsync(&ctx->h_state[2], ctx->state.p, sizeof(CgState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    take_stats(ctx, ctx->h_state[2]);
    return MAG_OK;
}

// ---- fused variant: one launch per CG iteration (cg.hip, k_cg_fused) ----
// interface slot tables of the multi-GPU exchange (k_comm_slots): where the q of an owned or a halo node sits in it
int ensure_qslots(mag_ctx *ctx)
{
    HIPCHK(ctx->own_qslot.reserve(4 * (size_t)ctx->N));
    HIPCHK(ctx->halo_qslot.reserve(4 * (size_t)std::max<int64_t>(ctx->halo_total, 1)));
    magk::comm_slots(ctx->iface.as<int32_t>(), ctx->n_iface, ctx->own0, ctx->own1, ctx->halo_g.as<int32_t>(),
                     ctx->halo_total, ctx->N, ctx->own_qslot.as<int32_t>(), ctx->halo_qslot.as<int32_t>(), ctx->stream);
    return MAG_OK;
}

// exchange buffers of the streaming kernels across ranks, one per parity: [nsums x g_all dot partials | q of the interface
// nodes].  Every rank computes the same g_all: same device, same cap, the most tiles of any rank.
int reserve_exchange(mag_ctx *ctx, int32_t g_all, int nsums)
{
    ctx->g_all = g_all;
    ctx->cwords = (size_t)nsums * g_all + 2 * (size_t)ctx->n_iface;
    HIPCHK(ctx->comm_f.reserve(8 * 2 * ctx->cwords + 64));
    return ensure_qslots(ctx);
}

// a fused launch's view of the exchange buffers: launch `par` reads the all-reduced buffer [par], fills buffer [par ^ 1]
template <class Params>
void set_exchange(const mag_ctx *ctx, int par, int nsums, Params &P)
{
    double *cin = ctx->comm_f.as<double>() + (size_t)par * ctx->cwords;
    double *cout = ctx->comm_f.as<double>() + (size_t)(par ^ 1) * ctx->cwords;
    P.part_in = cin;
    P.part_stride_in = ctx->g_all;
    P.nPart = ctx->g_all;
    P.part_out = cout;
    P.part_stride = ctx->g_all;
    P.comm_in_q = (const double2 *)(cin + (size_t)nsums * ctx->g_all);
    P.comm_out_q = (double2 *)(cout + (size_t)nsums * ctx->g_all);
    P.own_qslot = ctx->own_qslot.as<int32_t>();
    P.halo_qslot = ctx->halo_qslot.as<int32_t>();
}

// start of a fused solve (fp64 or fp32): init(part, stride) writes the b.b partials into partial buffer 0, then the state is
// set up from them.  One GPU: the kernel's own buffers of part_words sums per slot, `grid` slots.  Across ranks: exchange
// buffer 0 (its q part = q_{-1} = 0), summed over ranks in place.
template <class Init>
int setup_exchange(mag_ctx *ctx, int32_t grid, int part_words, Init init)
{
    using magk::FusedState;
    hipStream_t s = ctx->stream;
    const bool dist = ctx->dist;
    double *part = (dist ? ctx->comm_f : ctx->fpart).as<double>();
    const int32_t stride = dist ? ctx->g_all : magk::kMaxGrid;
    HIPCHK(hipMemsetAsync(part, 0, 8 * 2 * (dist ? ctx->cwords : (size_t)part_words * stride), s));
    init(part, stride);
    if (dist)
        if (int rc = allreduce(ctx, part, (int64_t)ctx->cwords)) return rc;
    magk::fused_setup(part, dist ? ctx->g_all : grid, stride, ctx->opt.stop_mode, ctx->opt.tol, (long long)ctx->opt.max_iter,
                      ctx->fstate.as<FusedState>(), s);
    if (dist && ctx->si) // tags of this solve's exchanges: sequence number << 24 + the launch counter (k_stream_exchange)
        HIPCHK(hipMemcpyAsync((char *)ctx->fstate.p + offsetof(FusedState, exchange_tag_base), &ctx->si_tag_base, 4,
                              hipMemcpyHostToDevice, s));
    return MAG_OK;
}

magk::FusedParams fused_params(mag_ctx *ctx, int par)
{
    magk::FusedParams P = {};
    const int32_t stride = magk::kMaxGrid;
    P.N = ctx->N;
    P.T = ctx->T;
    P.t0 = ctx->t0;
    P.t1 = ctx->t1;
    P.own0 = ctx->own0;
    P.own1 = ctx->own1;
    P.n_iface = ctx->n_iface;
    P.cap = ctx->cap;
    P.wt = 1; // write-through stores (the LDS-DMA kernel stores linear 1-KiB pieces; the AoS kernel ignores it)
    P.par = par;
    P.hist_len = ctx->opt.history_len;
    P.xyP = ctx->xyP.as<double2>();
    P.maskP = ctx->maskP.as<uint8_t>();
    P.meta = ctx->tmeta.as<magk::TileMeta>();
    P.ell16 = ctx->ell.as<uint32_t>();
    P.halo_g = ctx->halo_g.as<int32_t>();
    P.halo_xy = ctx->halo_xy.as<double2>();
    P.iface = ctx->iface.as<int32_t>();
    set_material(ctx, P);
    P.in = (par ? ctx->rqp1 : ctx->rqp0).as<magk::Rqp>();
    P.out = (par ? ctx->rqp0 : ctx->rqp1).as<magk::Rqp>();
    P.x = ctx->x.as<double2>();
    if (ctx->dist) {
        set_exchange(ctx, par, ctx->nsums(), P);
    } else {
        double *part = ctx->fpart.as<double>();
        P.part_out = part + (size_t)(par ^ 1) * 5 * stride;
        P.part_stride = stride;
        P.part_in = part + (size_t)par * 5 * stride;
        P.part_stride_in = stride;
        P.nPart = ctx->fgrid;
    }
    if (ctx->pre) {
        P.minvP = ctx->minvP.as<float4>();
        P.halo_minv = ctx->halo_minv.as<float4>();
    }
    P.st = ctx->fstate.as<magk::FusedState>();
    P.hist = ctx->hist.as<double>();
    return P;
}

int fused_block(mag_ctx *ctx, int G)
{
    for (int i = 0; i < G; ++i) {
        const magk::FusedParams P = fused_params(ctx, i & 1);
        magk::fused_launch(P, ctx->B, ctx->fgrid, ctx->stream);
        if (ctx->dist && ctx->si) {
            // the iteration's exchange through the device inboxes, in place on the buffer the launch just filled; its
            // epoch and tag come from the launch counter in FusedState, so the pair is the same node in every replay
            magk::stream_exchange_launch(P.part_out, ctx->g_all, ctx->n_iface, ctx->comm.rank, ctx->comm.nranks, ctx->own0,
                                         ctx->own1, i & 1, ctx->si_spin, ctx->iface.as<int32_t>(),
                                         ctx->iface_readers.as<uint8_t>(), ctx->inbox_peer,
                                         ctx->fstate.as<magk::FusedState>(), ctx->stream);
        } else if (ctx->dist) {
            // the iteration's ONE collective, in place on the buffer the launch just filled:
            // [r.r, p.q, r.q, q.q partials, slot by slot | q on interface nodes (owner's value + zeros)]
            if (int rc = allreduce(ctx, P.part_out, (int64_t)ctx->cwords)) return rc;
        }
    }
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

int reserve_fused(mag_ctx *ctx)
{
    HIPCHK(ctx->rqp0.reserve(sizeof(magk::Rqp) * (size_t)ctx->N));
    HIPCHK(ctx->rqp1.reserve(sizeof(magk::Rqp) * (size_t)ctx->N));
    HIPCHK(ctx->fpart.reserve(8 * 2 * 5 * (size_t)magk::kMaxGrid));
    HIPCHK(ctx->fstate.reserve(sizeof(magk::FusedState)));
    ctx->pre = ctx->opt.preconditioner != 0;
    if (ctx->pre) {
        // M = node-diagonal blocks of K_ff, inverted once per solve (16 bytes per node + per halo entry)
        HIPCHK(ctx->minvP.reserve(16 * (size_t)ctx->N));
        HIPCHK(ctx->halo_minv.reserve(16 * (size_t)std::max<int64_t>(ctx->halo_total, 1)));
        magk::precond_blocks(ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(), ctx->perm.as<uint32_t>(),
                             ctx->conn.as<int32_t>(), ctx->xy.as<double>(), ctx->uknown.as<uint8_t>(), ctx->N, ctx->nu,
                             ctx->youngs, ctx->thick, ctx->opt.preconditioner, ctx->minvP.as<float4>(), ctx->stream);
        magk::halo_minv(ctx->halo_g.as<int32_t>(), ctx->minvP.as<float4>(), ctx->halo_total,
                        ctx->halo_minv.as<float4>(), ctx->stream);
    }
    ctx->fgrid = magk::fused_grid(ctx->B, ctx->cap, ctx->t1 - ctx->t0, ctx->dist, ctx->pre);
    if (ctx->dist)
        return reserve_exchange(
            ctx, magk::fused_grid(ctx->B, ctx->cap, most_rank_tiles(ctx->T, ctx->comm.nranks), true, ctx->pre), ctx->nsums());
    return MAG_OK;
}

int ensure_fused_graph(mag_ctx *ctx, int G)
{
    mag_ctx::GraphKey k =
        graph_key(ctx, G, {ctx->x.p, ctx->rqp0.p, ctx->rqp1.p, ctx->fpart.p, ctx->fstate.p, ctx->hist.p, ctx->xyP.p,
                           ctx->maskP.p, ctx->tmeta.p, ctx->ell.p, ctx->halo_g.p, ctx->halo_xy.p, ctx->iface.p,
                           (void *)(intptr_t)ctx->cap, (void *)(intptr_t)(1 + ctx->fgrid) /* fused */,
                           ctx->pre ? ctx->minvP.p : nullptr, ctx->pre ? ctx->halo_minv.p : nullptr});
    if (ctx->dist) { // only the inbox exchange is captured (two kernels per iteration, no host work)
        void *dp[] = {ctx->comm_f.p, ctx->own_qslot.p, ctx->halo_qslot.p, ctx->iface_readers.p};
        for (int i = 0; i < 4; ++i) k.dptrs[i] = dp[i];
        for (int r = 0; r < 8; ++r) k.dptrs[4 + r] = ctx->inbox_peer[r];
        const int32_t dv[] = {1, ctx->g_all, ctx->n_iface, ctx->comm.rank, ctx->comm.nranks, ctx->own0, ctx->own1,
                              ctx->t0, ctx->t1, (int32_t)ctx->si_spin, (int32_t)ctx->cwords, ctx->nsums()};
        for (int i = 0; i < 12; ++i) k.d[i] = dv[i];
    }
    return capture_graph(ctx, k, [&] { return fused_block(ctx, G); });
}

int cg_phase_fused(mag_ctx *ctx)
{
    using magk::FusedState;
    hipStream_t s = ctx->stream;
    if (int rc = reserve_fused(ctx)) return rc;
    HIPCHK(hipMemsetAsync(ctx->x.p, 0, 16 * (size_t)ctx->N, s));
    ctx->si = false;
    if (ctx->dist) {
        // The per-iteration exchange goes through the device inboxes when they are open and this solve streams (the
        // mesh does not fit the chips, or the on-chip kernel is not wanted): k_stream_exchange instead of one RCCL
        // all-reduce per iteration.  Same decision on every rank: it depends on replicated quantities only.
        const int R = ctx->comm.nranks;
        ctx->si = R > 1 && R <= 8 && ctx->inbox_ready && !ctx->si_failed && !ctx->pre &&
                  env_int("MAG_TUNE_STREAM_INBOX", 1) != 0 &&
                  ctx->inbox_bytes >= 64 + 128 * (size_t)R + 64 * (size_t)ctx->n_iface &&
                  ctx->opt.max_iter < (int64_t(1) << 24) - 4;
        if (ctx->si) {
            ctx->si_tag_base = next_solve_seq(ctx) << 24;
            ctx->si_spin = (uint32_t)env_int("MAG_TUNE_STREAM_SPIN", 1 << 20); // tests: 0 forces the fallback
            // nothing of an earlier use of the inbox may look current: cleared before the all-reduce below lines the ranks up
            HIPCHK(hipMemsetAsync(ctx->inbox_own, 0, 64 + 128 * (size_t)R + 64 * (size_t)ctx->n_iface, s));
        }
    }
    if (int rc = setup_exchange(ctx, ctx->fgrid, 5, [&](double *part, int32_t stride) {
            magk::fused_init(ctx->bP.as<double2>(), ctx->pre ? ctx->minvP.as<float4>() : nullptr, ctx->rqp0.as<magk::Rqp>(),
                             ctx->rqp1.as<magk::Rqp>(), ctx->N, ctx->B, ctx->T, ctx->t0, ctx->t1, part, stride, ctx->fgrid, s);
        }))
        return rc;
    HIPCHK(hipGetLastError());

    const int G = ctx->opt.check_every;
    // one GPU, or several trading through the inboxes (iteration launch + k_stream_exchange, no host work): the block of G
    // iterations replays from a hipGraph; with an all-reduce per iteration the launches stay eager (RCCL's own enqueue)
    const bool graph = ctx->opt.use_graph != 0 && (!ctx->dist || ctx->si);
    if (graph)
        if (int rc = ensure_fused_graph(ctx, G)) return rc;
    ctx->exchange_kind = ctx->dist ? (ctx->si ? 3 : 1) : 0;
    if (int rc = run_blocks(ctx, ctx->fstate, ctx->h_fstate, [&] { return graph ? launch_graph(ctx) : fused_block(ctx, G); }))
        return rc;
    if (ctx->si) {
        // did any rank's exchange give up?  All ranks must agree before anyone changes path (as for the on-chip kernel)
        HIPCHK(hipMemcpyAsync(&ctx->h_fstate[2], ctx->fstate.p, sizeof(FusedState), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        bool gave_up = ctx->h_fstate[2].exchange_timeout || !ctx->h_fstate[2].done;
        if (int rc = any_rank(ctx, gave_up)) return rc;
        if (gave_up) {
            HIPCHK(hipMemsetAsync(ctx->inbox_own, 0, 64, s)); // the timeout word
            ctx->si_failed = true;
            ctx->exchange_timed_out = true;
            if (ctx->opt.verbose) printf("info: inbox exchange timed out, falling back to one all-reduce per iteration\n");
            return cg_phase_fused(ctx);
        }
    }
    if (ctx->dist)
        if (int rc = gather_solution(ctx)) return rc;
    HIPCHK(hipMemcpyAsync(&ctx->h_fstate[2], ctx->fstate.p, sizeof(FusedState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    take_stats(ctx, ctx->h_fstate[2]);
    return MAG_OK;
}

// ---- on-chip variant: ONE launch for the whole solve (persist_kernel.h, k_cg_persist) ----
// Which instantiation (mode): edge blocks in registers when every row of the mesh is one short fan (1; k_ring16 left the
// answer behind tile_rdeg's two arrays), the triangle walk with cached weights otherwise (0).  One 4-byte read per solve.
// Round 4: a mesh whose rows are single fans of ANY length (flag word 1: gmsh-type meshes, a quarter of their nodes with
// seven neighbours) runs the edge-block kernel too, the blocks beyond six per node as 32-byte records in an LDS pool -- if
// every workgroup's records fit the LDS its more compact layout leaves free (2; P then carries the pool); the walk otherwise.
// (several ranks: the ordering phase is replicated, so every rank reads the same flag.  The multi-GPU edge-block
// instantiation is the default since round 4 -- two ranks sharing the GPU at four tiles per workgroup: 9.1 against 10.7 us
// per iteration, fixture parity on both ranks --; MAG_TUNE_PERSIST_MG_BLOCKS=0 keeps the triangle walk across ranks)
int choose_edge_blocks(mag_ctx *ctx, bool mg, magk::PersistParams &P, int &mode)
{
    hipStream_t s = ctx->stream;
    mode = 0;
    if ((mg && env_int("MAG_TUNE_PERSIST_MG_BLOCKS", 1) == 0) || getenv("MAG_TUNE_PERSIST_TRIANGLES")) return MAG_OK;
    int32_t fan_flags = 3;
    if (ctx->order_sharded) { // (this rank's ring words cover its own tiles only: the ordering phase has OR-ed the flags over the ranks)
        fan_flags = ctx->fan_flags_global;
    } else {
        HIPCHK(hipMemcpyAsync(&fan_flags, ctx->tile_rdeg.as<int32_t>() + 2 * (size_t)ctx->T, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if (fan_flags == 0) mode = 1;
    if (!((fan_flags == 1 && env_int("MAG_TUNE_PERSIST_NO_OVERFLOW", 0) == 0) ||
          (fan_flags == 0 && getenv("MAG_TUNE_PERSIST_FORCE_OVERFLOW"))) ||
        (mg && env_int("MAG_TUNE_PERSIST_MG_OVERFLOW", 1) == 0)) // =0: several ranks keep the triangle walk on such meshes
        return MAG_OK;
    // per-node overflow counts -> scan -> the limits the LDS must meet
    const int nb = magk::persist_block_entries();
    const int64_t npad = (int64_t)ctx->T * ctx->B;
    HIPCHK(ctx->ovf_cnt.reserve(4 * ((size_t)npad + 1)));
    HIPCHK(ctx->ovf_off.reserve(4 * ((size_t)npad + 1) + 16));
    magk::ovf_counts(ctx->row_info.as<uint8_t>(), npad, nb, ctx->ovf_cnt.as<int32_t>(), s);
    if (int rc = scan_i32(ctx, ctx->ovf_cnt.as<int32_t>(), ctx->ovf_off.as<int32_t>(), (size_t)npad + 1)) return rc;
    int32_t *lim_d = ctx->ovf_cnt.as<int32_t>(); // (the counts are not needed after the scan: their first words hold the limits)
    HIPCHK(hipMemsetAsync(lim_d, 0, 8, s));
    // (several ranks: the limits over EVERY rank's workgroups -- the ordering phase is replicated --, so that all ranks reach
    // the same decision; sharded ordering phase: only the own tiles' rows are known here -- the ranks vote below)
    const int R = ctx->comm.nranks;
    for (int r_ = 0; r_ < R; ++r_) {
        if (ctx->order_sharded && r_ != ctx->comm.rank) continue;
        magk::ovf_limits(ctx->ovf_off.as<int32_t>(), ctx->B, ctx->persist_k, rank_tile_lo(ctx->T, R, r_),
                         rank_tile_lo(ctx->T, R, r_ + 1), lim_d, s);
    }
    int32_t lim[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(lim, lim_d, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&lim[2], ctx->ovf_off.as<int32_t>() + npad, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int32_t pool = ((lim[0] + 1 + 7) / 8) * 8; // + record 0, the zero block
    // 12 bits of pool position and 4 bits of count per node slot; the kernel's static LDS on top of the dynamic
    bool walk = !(lim[0] + 1 <= 4095 && lim[1] <= 15 &&
                  magk::persist_lds_bytes(ctx->B, ctx->cap, ctx->persist_maxh, 2, pool, mg) + 256 <=
                      160 * 1024);
    // one instantiation for all ranks: a rank whose pool does not fit sends everybody to the walk
    if (ctx->order_sharded)
        if (int rc = any_rank(ctx, walk)) return rc;
    if (walk) {
        if (ctx->opt.verbose)
            printf("info: edge blocks with overflow do not fit (%d records in a workgroup, %d at a node): triangle walk\n", lim[0], lim[1]);
        return MAG_OK;
    }
    mode = 2;
    P.pool_cap = pool;
    ctx->ovf_total = lim[2];
    HIPCHK(ctx->ovf_rec.reserve(32 * (size_t)std::max(lim[2], 1)));
    P.row_info = ctx->row_info.as<uint8_t>();
    P.ovf_off = ctx->ovf_off.as<int32_t>();
    P.ovf_rec = ctx->ovf_rec.as<double>();
    return MAG_OK;
}

// what every launch of the on-chip kernel is told about the mesh, the stop rule and the context's single-case buffers
void persist_common_params(mag_ctx *ctx, bool mg, magk::PersistParams &P)
{
    P.N = ctx->N;
    P.T = ctx->T;
    P.tiles_per_wg = ctx->persist_k;
    P.cap = ctx->cap;
    P.maxh = ctx->persist_maxh;
    P.hist_len = ctx->opt.history_len;
    P.stop_mode = ctx->opt.stop_mode;
    // ~0.3 s of polling (each poll is a memory round trip) before a workgroup concludes that the grid is not resident;
    // several ranks start apart: a longer budget
    P.spin_limit = (uint32_t)env_int("MAG_TUNE_PERSIST_SPIN", mg ? 1 << 21 : 1 << 19);
    P.max_iter = (long long)ctx->opt.max_iter;
    P.tol = ctx->opt.tol;
    set_material(ctx, P);
    P.xyP = ctx->xyP.as<double2>();
    P.maskP = ctx->maskP.as<uint8_t>();
    P.meta = ctx->tmeta.as<magk::TileMeta>();
    P.ell16 = ctx->ell.as<uint32_t>();
    P.halo_g = ctx->halo_g.as<int32_t>();
    P.halo_xy = ctx->halo_xy.as<double2>();
    P.bP = ctx->bP.as<double2>();
    P.x = ctx->x.as<double2>();
    P.qg = ctx->qx.as<unsigned long long>();
    P.recg = ctx->wg_part.as<unsigned long long>();
    P.sync = ctx->psync.as<uint32_t>();
    P.st = ctx->fstate.as<magk::FusedState>();
    P.hist = ctx->hist.as<double>();
}

// the instantiation for this mesh (mag_stats.edge_blocks), the nodes read through memory, the nodes' blocks: once per solve --
// or once for all load cases: none of it depends on the prescribed values.  build = false (design variants): the instantiation and
// the marks only -- they follow from the ring tables --, the caller builds every variant's blocks from its own coordinates
int persist_prepare_blocks(mag_ctx *ctx, bool mg, magk::PersistParams &P, int &eb_mode, bool build = true)
{
    hipStream_t s = ctx->stream;
    eb_mode = 0;
    if (int rc = choose_edge_blocks(ctx, mg, P, eb_mode)) return rc;
    ctx->edge_blocks = eb_mode;
    // which nodes are read through memory at all by this rank's tiles, with persist_k tiles per workgroup (the others publish
    // nothing on this GPU; what other ranks read goes through the inboxes)
    magk::mark_external(ctx->halo_g.as<int32_t>(), ctx->tmeta.as<magk::TileMeta>(), ctx->t0, ctx->t1, ctx->B, ctx->persist_k,
                        ctx->maskP.as<uint8_t>(), eb_mode == 2, s);
    if (eb_mode && build) { // the nodes' blocks, once per solve (18 doubles per node of the padded order, value-major)
        const int64_t npad = (int64_t)ctx->T * ctx->B;
        HIPCHK(ctx->kblocks.reserve(8 * (size_t)(3 * magk::persist_block_entries()) * (size_t)npad));
        P.kblocks = ctx->kblocks.as<double>();
        P.kb_stride = npad;
        magk::edge_blocks_build(P, ctx->B, ctx->kblocks.as<double>(), eb_mode, 0, s);
    }
    return MAG_OK;
}

// a workgroup gave up waiting at the grid barrier (not every workgroup resident: the GPU is shared with another process, or
// fewer CUs are usable than reported): use the streaming kernels from now on
void persist_back_off(mag_ctx *ctx)
{
    ctx->persist_failed = true;
    ctx->persist_timed_out = true;
    ctx->persist_backoff = ctx->persist_backoff ? std::min(2 * ctx->persist_backoff, 1024) : 8;
    ctx->persist_retry_in = ctx->persist_backoff;
    ctx->persist = false;
    if (ctx->opt.verbose) printf("info: on-chip CG not co-resident, falling back to the streaming iteration\n");
}

int cg_phase_persist(mag_ctx *ctx)
{
    using magk::FusedState;
    hipStream_t s = ctx->stream;
    const int grid = ctx->persist_grid;
    HIPCHK(ctx->fstate.reserve(sizeof(FusedState)));
    const size_t qg_bytes = 2 * 32 * (size_t)ctx->N, rec_bytes = 2 * 64 * (size_t)grid;
    HIPCHK(ctx->qx.reserve(qg_bytes));
    HIPCHK(ctx->wg_part.reserve(rec_bytes));
    HIPCHK(ctx->psync.reserve(64));
    // tags of a previous solve must not look current: granules and the timeout word are zeroed before EVERY launch
    HIPCHK(hipMemsetAsync(ctx->qx.p, 0, qg_bytes, s));
    HIPCHK(hipMemsetAsync(ctx->wg_part.p, 0, rec_bytes, s));
    HIPCHK(hipMemsetAsync(ctx->psync.p, 0, 64, s));
    HIPCHK(hipMemsetAsync(ctx->fstate.p, 0, sizeof(FusedState), s));
    const int R = ctx->comm.nranks;
    const bool mg = R > 1;
    magk::PersistParams P = {};
    P.nranks = 1;
    if (mg) {
        // interface slot tables (as the streaming multi-GPU path uses them), the republished-sums record, the window
        if (int rc = ensure_qslots(ctx)) return rc;
        HIPCHK(ctx->grec.reserve(2 * 64));
        HIPCHK(hipMemsetAsync(ctx->grec.p, 0, 2 * 64, s));
        // The window is never zeroed: tags carry the solve's sequence number (same on every rank: all ranks run the
        // same solves) above 24 bits of iteration count, so nothing of an earlier solve can look current (every solve
        // overwrites the slots of the one before; 255 sequence numbers go round).
        P.tag_base = next_solve_seq(ctx) << 24;
        P.t0 = ctx->t0;
        P.t1 = ctx->t1;
        P.rank = ctx->comm.rank;
        P.nranks = R;
        P.n_iface = ctx->n_iface;
        P.own_qslot = ctx->own_qslot.as<int32_t>();
        P.halo_qslot = ctx->halo_qslot.as<int32_t>();
        P.win_shared = ctx->inbox_ready ? 0 : 1;
        for (int r = 0; r < R; ++r)
            P.inbox[r] = (uint8_t *)(ctx->inbox_ready ? ctx->inbox_peer[r] : ctx->win_dev);
        P.iface_readers = ctx->iface_readers.as<uint8_t>();
        P.grec = ctx->grec.as<unsigned long long>();
        // device inboxes: one extra workgroup carries the rank-level exchange (persist_comm_loop) when a CU is free for
        // it on every rank -- the grids differ by at most one workgroup, so the largest decides for all
        int cus = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
        const int32_t grid_max = (most_rank_tiles(ctx->T, R) + ctx->persist_k - 1) / ctx->persist_k;
        P.comm_wg = (ctx->inbox_ready && grid_max + 1 <= cus) ? 1 : 0;
    }
    persist_common_params(ctx, mg, P);
    if (mg) {
        // every rank's kernel must be running before anybody's spin budget runs out: line the streams up first
        // Nothing of an earlier use may look current: a window handed over from another context, or slots of the solve
        // 255 sequence numbers ago, could carry this solve's tags.  Every rank clears the extent of ITS inbox this solve
        // will use (rank 0 the shared host window) before the line-up all-reduce: nobody stores into an inbox before
        // every rank has passed that all-reduce, i.e. after every clear.
        {
            const size_t used = 64 + 128 * (size_t)R + 64 * (size_t)ctx->n_iface;
            if (ctx->inbox_ready)
                HIPCHK(hipMemsetAsync(ctx->inbox_own, 0, used, s));
            else if (ctx->comm.rank == 0)
                HIPCHK(hipMemsetAsync(ctx->win_dev, 0, used, s));
        }
        HIPCHK(hipMemsetAsync(ctx->comm_pq.p, 0, 8, s));
        if (int rc = allreduce(ctx, ctx->comm_pq.as<double>(), 1)) return rc;
    }
    const bool stamps = magk::persist_stamps_built() && getenv("MAG_TUNE_PERSIST_STAMPS") != nullptr;
    if (stamps) { // diagnostic build only (scripts/persist_phases.sh): phase times per workgroup
        HIPCHK(ctx->pstamps.reserve(8 * (size_t)magk::persist_stamp_words() * (size_t)(grid + 1)));
        HIPCHK(hipMemsetAsync(ctx->pstamps.p, 0, 8 * (size_t)magk::persist_stamp_words() * (size_t)(grid + 1), s));
        P.stamps = ctx->pstamps.as<unsigned long long>();
    }
    int eb_mode = 0;
    if (int rc = persist_prepare_blocks(ctx, mg, P, eb_mode)) return rc;
    if (!magk::persist_launch(P, ctx->B, grid + P.comm_wg, 1, magk::PERSIST_SINGLE, eb_mode, s))
        return fail(ctx, MAG_ERR_STATE, "on-chip CG: no kernel for this shape");
    if (stamps) {
        // (several ranks: one file per rank, "<name>.<rank>"; with an exchange workgroup its row follows the compute workgroups')
        const int rows = grid + P.comm_wg;
        std::vector<unsigned long long> h((size_t)magk::persist_stamp_words() * (size_t)rows);
        HIPCHK(hipMemcpyAsync(h.data(), ctx->pstamps.p, 8 * h.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::string fname = getenv("MAG_TUNE_PERSIST_STAMPS");
        if (mg) fname += "." + std::to_string(ctx->comm.rank);
        if (FILE *f = fopen(fname.c_str(), "w")) {
            for (int g = 0; g < rows; ++g) {
                for (int k = 0; k < magk::persist_stamp_words(); ++k)
                    fprintf(f, "%s%llu", k ? "," : "", h[(size_t)g * magk::persist_stamp_words() + k]);
                fprintf(f, "\n");
            }
            fclose(f);
        }
    }
    HIPCHK(hipGetLastError());
    uint32_t h_sync[16] = {};
    HIPCHK(hipMemcpyAsync(&ctx->h_fstate[2], ctx->fstate.p, sizeof(FusedState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_sync, ctx->psync.p, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const FusedState &st = ctx->h_fstate[2];
    bool failed = h_sync[9] != 0 || !st.done;
    if (mg) { // all ranks must agree before anyone changes path
        if (int rc = any_rank(ctx, failed)) return rc;
        if (failed) { // the timeout word, for the next context
            if (ctx->inbox_ready)
                HIPCHK(hipMemsetAsync(ctx->inbox_own, 0, 64, s));
            else
                *(volatile uint32_t *)ctx->win_host = 0;
        }
    }
    if (failed) {
        persist_back_off(ctx);
        ctx->cg_kernel = 1;
        return cg_phase_fused(ctx);
    }
    ctx->cg_kernel = 2;
    ctx->persist_backoff = 0; // co-resident again: the next failure starts from the short wait
    ctx->exchange_kind = mg ? 2 : 0;
    if (mg) { // every rank returns the whole solution
        if (int rc = gather_solution(ctx)) return rc;
        HIPCHK(hipStreamSynchronize(s));
    }
    take_stats(ctx, st);
    return MAG_OK;
}

// solver.rs:365-404,427-432,123-137 on the device: K_ff (exact zeros dropped) + b in compact unknown numbering
// (kval: the matrix in K's pattern -- ctx->kval, or the transient pass's A; rhs: b = f_in - K u_in of the uploaded problem too)
int build_reduced(mag_ctx *ctx, bool fill, const double *kval = nullptr, bool rhs = true)
{
    if (!kval) kval = ctx->kval.as<double>();
    const int64_t N = ctx->N, n = 2 * N;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx->isfree.reserve(4 * ((size_t)n + 1)));
    HIPCHK(ctx->fidx.reserve(4 * ((size_t)n + 1)));
    HIPCHK(ctx->rcnt.reserve(4 * ((size_t)n + 1)));
    HIPCHK(ctx->rowoff.reserve(4 * ((size_t)n + 1)));
    magk::free_flags(ctx->uknown.as<uint8_t>(), n, ctx->isfree.as<int32_t>(), s);
    if (int rc = scan_i32(ctx, ctx->isfree.as<int32_t>(), ctx->fidx.as<int32_t>(), (size_t)n + 1)) return rc;
    magk::reduce_count(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), kval,
                       ctx->uknown.as<uint8_t>(), N, ctx->rcnt.as<int32_t>(), s);
    if (int rc = scan_i32(ctx, ctx->rcnt.as<int32_t>(), ctx->rowoff.as<int32_t>(), (size_t)n + 1)) return rc;
    int32_t h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&h[0], ctx->fidx.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h[1], ctx->rowoff.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ctx->nf = h[0];
    ctx->nz_ff = h[1];
    ctx->stats.n_free = ctx->nf;
    if (ctx->nf == 0) return fail(ctx, MAG_ERR_BC_MISMATCH, "no unknown displacement in the boundary-condition set");
    if (!fill) return MAG_OK;
    const int64_t nf = ctx->nf, nz = ctx->nz_ff;
    HIPCHK(ctx->rp_ff.reserve(4 * ((size_t)nf + 1)));
    HIPCHK(ctx->col_ff.reserve(4 * (size_t)(nz > 0 ? nz : 1)));
    HIPCHK(ctx->val_ff.reserve(8 * (size_t)(nz > 0 ? nz : 1)));
    HIPCHK(ctx->b_ff.reserve(8 * (size_t)nf));
    magk::reduce_fill(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), kval,
                      ctx->uknown.as<uint8_t>(), ctx->fidx.as<int32_t>(), ctx->rowoff.as<int32_t>(), N,
                      ctx->rp_ff.as<int32_t>(), ctx->col_ff.as<int32_t>(), ctx->val_ff.as<double>(), s);
    if (rhs)
        magk::rhs_compact(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), kval,
                          ctx->uknown.as<uint8_t>(), ctx->uin.as<double>(), ctx->fin.as<double>(),
                          ctx->fidx.as<int32_t>(), N, ctx->b_ff.as<double>(), s);
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

// MAG_OP_CSR: the reference's own iteration (CSR SpMV on K_ff + argmin recurrences), three launches per iteration
// (reduced: the reduced system and its right-hand side are in place -- the transient pass's, built once per run of the pass;
// known / u_out: the values of the prescribed DOFs and where the expanded solution goes)
int cg_phase_csr(mag_ctx *ctx, bool reduced = false, const double *known = nullptr, double *u_out = nullptr)
{
    hipStream_t s = ctx->stream;
    if (ctx->comm.distributed()) return fail(ctx, MAG_ERR_BAD_ARGS, "cg_operator MAG_OP_CSR is single-GPU only");
    if (!reduced)
        if (int rc = build_reduced(ctx, true)) return rc;
    const int64_t nf = ctx->nf;
    const size_t vb = 8 * (size_t)nf;
    double *x = ctx->x.as<double>(), *r = ctx->r.as<double>(), *q = ctx->q.as<double>();
    HIPCHK(hipMemsetAsync(x, 0, vb, s));
    HIPCHK(hipMemsetAsync(ctx->p0.p, 0, vb, s));
    HIPCHK(hipMemsetAsync(ctx->p1.p, 0, vb, s));
    magk::csr_init(ctx->b_ff.as<double>(), r, nf, ctx->partRR.as<double>(), s);
    const int grid = magk::csr_grid(nf);
    magk::cg_setup(ctx->partRR.as<double>(), grid, ctx->opt.stop_mode, ctx->opt.tol, (long long)ctx->opt.max_iter,
                   ctx->state.as<CgState>(), s);
    HIPCHK(hipGetLastError());
    int G = ctx->tr_first_block > 0 ? ctx->tr_first_block : ctx->opt.check_every;
    auto block = [&]() -> int {
        const int len = G;
        G = ctx->opt.check_every;
        for (int i = 0; i < len; ++i) {
            magk::CsrCgParams P = {};
            P.n = nf;
            P.nPart = grid;
            P.hist_len = ctx->opt.history_len;
            P.rowptr = ctx->rp_ff.as<int32_t>();
            P.col = ctx->col_ff.as<int32_t>();
            P.val = ctx->val_ff.as<double>();
            P.x = x;
            P.r = r;
            P.pprev = (i & 1) ? ctx->p0.as<double>() : ctx->p1.as<double>();
            P.pnew = (i & 1) ? ctx->p1.as<double>() : ctx->p0.as<double>();
            P.q = q;
            P.partRR = ctx->partRR.as<double>();
            P.partPQ = ctx->partPQ.as<double>();
            P.st = ctx->state.as<CgState>();
            P.hist = ctx->hist.as<double>();
            magk::csr_p_launch(P, s);
            magk::csr_spmv_launch(P, s);
            magk::csr_update_launch(nf, r, q, ctx->partPQ.as<double>(), grid, ctx->partRR.as<double>(),
                                    ctx->state.as<CgState>(), s);
        }
        HIPCHK(hipGetLastError());
        return MAG_OK;
    };
    if (int rc = run_blocks(ctx, ctx->state, ctx->h_state, block)) return rc;
    HIPCHK(hipMemcpyAsync(&ctx->h_state[2], ctx->state.p, sizeof(CgState), hipMemcpyDeviceToHost, s));
    // solver.rs:443-454: the solution goes back into the unknown slots in ascending DOF order
    magk::expand_free(x, ctx->fidx.as<int32_t>(), ctx->uknown.as<uint8_t>(), known ? known : ctx->uin.as<double>(), 2 * ctx->N,
                      u_out ? u_out : ctx->u.as<double>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    take_stats(ctx, ctx->h_state[2]);
    return MAG_OK;
}

// ---- mag_options.field_cg: one fused launch per iteration over the assembled K's block rows (cg.hip, k_cg_field) ----
// cg_phase_fused's protocol on one GPU: the right-hand side in bP is in Hilbert numbering already, the solution stays in
// ctx->x; the reduced system (build_reduced) is not needed and not built.
// the matrix of a solve: the block-row table, the gathered values and the inverse blocks -- a field's K (field_system), or the
// transient pass's A
struct FieldSystem {
    const magk::FieldTileMeta *meta;
    const uint16_t *slot;
    const double2 *fval;
    const float4 *minvP, *halo_minv; // null: plain CG
    int64_t total;
    int32_t grid;
};

FieldSystem field_system(const mag_ctx *ctx)
{
    const bool pre = ctx->opt.field_cg >= 2;
    return {ctx->fc_meta.as<magk::FieldTileMeta>(), ctx->fc_slot.as<uint16_t>(), ctx->fc_val.as<double2>(),
            pre ? ctx->minvP.as<float4>() : nullptr, pre ? ctx->halo_minv.as<float4>() : nullptr, ctx->fc_total, ctx->fc_grid};
}

magk::FieldCgParams field_cg_params(mag_ctx *ctx, int par, const FieldSystem &sys)
{
    magk::FieldCgParams P = {};
    const int32_t stride = magk::kMaxGrid;
    P.N = ctx->N;
    P.total = sys.total;
    P.T = ctx->T;
    P.nPart = sys.grid;
    P.cap = ctx->cap;
    P.par = par;
    P.hist_len = ctx->opt.history_len;
    P.part_stride = stride;
    P.maskP = ctx->maskP.as<uint8_t>();
    P.meta = sys.meta;
    P.slot = sys.slot;
    P.fval = sys.fval;
    P.halo_g = ctx->halo_g.as<int32_t>();
    P.in = (par ? ctx->rqp1 : ctx->rqp0).as<magk::Rqp>();
    P.out = (par ? ctx->rqp0 : ctx->rqp1).as<magk::Rqp>();
    P.x = ctx->x.as<double2>();
    double *part = ctx->fpart.as<double>();
    P.part_in = part + (size_t)par * 5 * stride;
    P.part_out = part + (size_t)(par ^ 1) * 5 * stride;
    P.st = ctx->fstate.as<magk::FusedState>();
    P.hist = ctx->hist.as<double>();
    P.minvP = sys.minvP;
    P.halo_minv = sys.halo_minv;
    return P;
}

int field_cg_block(mag_ctx *ctx, int G, const FieldSystem &sys)
{
    for (int i = 0; i < G; ++i) magk::field_cg_launch(field_cg_params(ctx, i & 1, sys), ctx->B, sys.grid, ctx->stream);
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

int cg_phase_field(mag_ctx *ctx, const FieldSystem &sys)
{
    using magk::FusedState;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx->rqp0.reserve(sizeof(magk::Rqp) * (size_t)ctx->N));
    HIPCHK(ctx->rqp1.reserve(sizeof(magk::Rqp) * (size_t)ctx->N));
    HIPCHK(ctx->fpart.reserve(8 * 2 * 5 * (size_t)magk::kMaxGrid));
    HIPCHK(ctx->fstate.reserve(sizeof(FusedState)));
    HIPCHK(hipMemsetAsync(ctx->x.p, 0, 16 * (size_t)ctx->N, s));
    double *part = ctx->fpart.as<double>();
    const int32_t stride = magk::kMaxGrid, grid = sys.grid;
    HIPCHK(hipMemsetAsync(part, 0, 8 * 2 * 5 * (size_t)stride, s));
    magk::fused_init(ctx->bP.as<double2>(), sys.minvP, ctx->rqp0.as<magk::Rqp>(),
                     ctx->rqp1.as<magk::Rqp>(), ctx->N, ctx->B, ctx->T, 0, ctx->T, part, stride, grid, s);
    magk::fused_setup(part, grid, stride, ctx->opt.stop_mode, ctx->opt.tol, (long long)ctx->opt.max_iter,
                      ctx->fstate.as<FusedState>(), s);
    HIPCHK(hipGetLastError());

    const int G = ctx->opt.check_every;
    const bool graph = ctx->opt.use_graph != 0;
    if (graph) {
        const mag_ctx::GraphKey k =
            graph_key(ctx, G, {ctx->x.p, ctx->rqp0.p, ctx->rqp1.p, ctx->fpart.p, ctx->fstate.p, ctx->hist.p, ctx->maskP.p,
                               (void *)sys.meta, (void *)sys.slot, (void *)sys.fval, ctx->halo_g.p, (void *)(intptr_t)ctx->cap,
                               (void *)(intptr_t)(0x10000 + sys.grid) /* block rows */, (void *)(intptr_t)sys.total,
                               (void *)sys.minvP, (void *)sys.halo_minv});
        if (int rc = capture_graph(ctx, k, [&] { return field_cg_block(ctx, G, sys); })) return rc;
    }
    int first = ctx->tr_first_block; // (the transient pass's, launched one by one: no graph)
    auto eager = [&] {
        const int len = first > 0 ? first : G;
        first = 0;
        return field_cg_block(ctx, len, sys);
    };
    if (int rc = run_blocks(ctx, ctx->fstate, ctx->h_fstate, [&] { return graph ? launch_graph(ctx) : eager(); })) return rc;
    HIPCHK(hipMemcpyAsync(&ctx->h_fstate[2], ctx->fstate.p, sizeof(FusedState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    take_stats(ctx, ctx->h_fstate[2]);
    return MAG_OK;
}

// ---- fp32 leg of BASELINE config 5: same fused iteration, CG state and operator arithmetic in fp32 (cg.hip, k_cg_fused32) ----
magk::Fused32Params fused32_params(mag_ctx *ctx, int par, int grid)
{
    magk::Fused32Params P = {};
    const int32_t stride = magk::kMaxGrid;
    P.N = ctx->N;
    P.T = ctx->T;
    P.cap = ctx->cap;
    P.par = par;
    P.hist_len = ctx->opt.history_len;
    P.xyP32 = ctx->xy32.as<float2>();
    P.maskP = ctx->maskP.as<uint8_t>();
    P.meta = ctx->tmeta.as<magk::TileMeta>();
    P.ell16 = ctx->ell.as<uint32_t>();
    P.halo_g = ctx->halo_g.as<int32_t>();
    P.halo_xy32 = ctx->hxy32.as<float2>();
    set_material(ctx, P);
    P.in = (par ? ctx->rqp32b : ctx->rqp32a).as<magk::Rqp32>();
    P.out = (par ? ctx->rqp32a : ctx->rqp32b).as<magk::Rqp32>();
    P.x = ctx->x32.as<float2>();
    if (ctx->dist) { // (one GPU: the range fields stay zero)
        P.t0 = ctx->t0;
        P.t1 = ctx->t1;
        P.own0 = ctx->own0;
        P.own1 = ctx->own1;
        P.n_iface = ctx->n_iface;
        P.iface = ctx->iface.as<int32_t>();
        set_exchange(ctx, par, 4, P);
    } else {
        P.nPart = grid;
        P.part_in = ctx->fpart.as<double>() + (size_t)par * 4 * stride;
        P.part_out = ctx->fpart.as<double>() + (size_t)(par ^ 1) * 4 * stride;
        P.part_stride = stride;
    }
    P.st = ctx->fstate.as<magk::FusedState>();
    P.hist = ctx->hist.as<double>();
    return P;
}

int cg_phase_fused32(mag_ctx *ctx)
{
    using magk::FusedState;
    hipStream_t s = ctx->stream;
    if (!ctx->use_lds || ctx->B == 1024)
        return fail(ctx, MAG_ERR_BAD_ARGS, "precision fp32 needs the LDS-halo operator and tile_nodes 256|512");
    const int64_t N = ctx->N;
    const int32_t stride = magk::kMaxGrid;
    HIPCHK(ctx->xy32.reserve(8 * (size_t)N));
    HIPCHK(ctx->hxy32.reserve(8 * (size_t)std::max<int64_t>(ctx->halo_total, 1)));
    HIPCHK(ctx->rqp32a.reserve(sizeof(magk::Rqp32) * (size_t)N));
    HIPCHK(ctx->rqp32b.reserve(sizeof(magk::Rqp32) * (size_t)N));
    HIPCHK(ctx->x32.reserve(8 * (size_t)N));
    HIPCHK(ctx->fpart.reserve(8 * 2 * 4 * (size_t)stride));
    HIPCHK(ctx->fstate.reserve(sizeof(FusedState)));
    magk::coords32(ctx->xyP.as<double>(), ctx->halo_g.as<int32_t>(), ctx->tile_hoff.as<int32_t>(), N, ctx->B, ctx->T,
                   ctx->xy32.as<float>(), ctx->hxy32.as<float>(), s);
    const int grid = magk::fused32_grid(ctx->B, ctx->cap, ctx->t1 - ctx->t0);
    if (ctx->dist) {
        // the streaming protocol of cg_phase_fused, in fp32: the exchange buffer stays in doubles, one in-place all-reduce
        // per iteration
        ctx->pre = false;
        if (int rc = reserve_exchange(ctx, magk::fused32_grid(ctx->B, ctx->cap, most_rank_tiles(ctx->T, ctx->comm.nranks)), 4))
            return rc;
    }
    // (one GPU: ctx->t0 = 0, ctx->t1 = T)
    if (int rc = setup_exchange(ctx, grid, 4, [&](double *part, int32_t stride) {
            magk::fused32_init(ctx->bP.as<double2>(), ctx->rqp32a.as<magk::Rqp32>(), ctx->rqp32b.as<magk::Rqp32>(),
                               ctx->x32.as<float2>(), N, ctx->B, ctx->T, ctx->t0, ctx->t1, part, stride, grid, s);
        }))
        return rc;
    HIPCHK(hipGetLastError());
    const int G = ctx->opt.check_every;
    auto block = [&]() -> int {
        for (int i = 0; i < G; ++i) {
            const magk::Fused32Params P = fused32_params(ctx, i & 1, grid);
            magk::fused32_launch(P, ctx->B, grid, s);
            if (ctx->dist)
                if (int rc = allreduce(ctx, P.part_out, (int64_t)ctx->cwords)) return rc;
        }
        HIPCHK(hipGetLastError());
        return MAG_OK;
    };
    if (int rc = run_blocks(ctx, ctx->fstate, ctx->h_fstate, block)) return rc;
    magk::x32_to_f64(ctx->x32.as<float2>(), N, ctx->x.as<double2>(), s);
    if (ctx->dist)
        if (int rc = gather_solution(ctx)) return rc;
    HIPCHK(hipMemcpyAsync(&ctx->h_fstate[2], ctx->fstate.p, sizeof(FusedState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    take_stats(ctx, ctx->h_fstate[2]);
    return MAG_OK;
}

// The timing helpers (mag_time_operator / mag_time_spmv) need the symbolic phase and the CG buffers, not a solve: after
// a completed mag_run everything is in place; straight after mag_upload the tables are built here and the vectors
// zeroed (bench.py's HBM-resident leg times the kernels on the 16M-triangle mesh without paying for its 20 000
// iterations).
int prepare_timing(mag_ctx *ctx)
{
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "no problem uploaded");
    if (ctx->have_order && ctx->x.p && ctx->tmpP.p) return MAG_OK;
    if (int rc = ensure_order(ctx)) return rc;
    if (int rc = reserve_cg(ctx)) return rc;
    const size_t vb = 16 * (size_t)ctx->N;
    hipStream_t s = ctx->stream;
    for (DevBuf *b : {&ctx->x, &ctx->r, &ctx->p0, &ctx->p1, &ctx->q, &ctx->tmpP}) HIPCHK(hipMemsetAsync(b->p, 0, vb, s));
    if (ctx->fused) {
        if (int rc = reserve_fused(ctx)) return rc;
        HIPCHK(hipMemsetAsync(ctx->rqp0.p, 0, sizeof(magk::Rqp) * (size_t)ctx->N, s));
        HIPCHK(hipMemsetAsync(ctx->rqp1.p, 0, sizeof(magk::Rqp) * (size_t)ctx->N, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

double ev_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.0;
    return (double)ms;
}

// ms per call of launch(): 3 warm-up calls, then reps calls between events 8 and 9
template <class Launch>
int time_launches(mag_ctx *ctx, int32_t reps, Launch launch, double *ms_out)
{
    hipStream_t s = ctx->stream;
    for (int i = 0; i < 3; ++i)
        if (int rc = launch()) return rc;
    HIPCHK(hipEventRecord(ctx->ev[8], s));
    for (int i = 0; i < reps; ++i)
        if (int rc = launch()) return rc;
    HIPCHK(hipEventRecord(ctx->ev[9], s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    *ms_out = ev_ms(ctx->ev[8], ctx->ev[9]) / reps;
    return MAG_OK;
}

} // namespace

// ======================================================================= C ABI

extern "C" {

int mag_version(void) { return MAG_ABI_VERSION; }

void mag_default_options(mag_options *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->device = 0;
    o->stop_mode = MAG_STOP_RNORM;
    o->tol = MAG_TARGET_CG_COST;
    o->max_iter = MAG_MAX_CG_ITER;
    o->cg_operator = MAG_OP_MATRIX_FREE;
    o->assemble_csr = 1;
    o->check_every = 64;
    o->use_graph = 1;
    o->tile_nodes = 0;
    o->history_len = 0;
    o->verbose = 0;
    o->op_variant = 0;
    o->cg_variant = 2;
    o->precision = 0;
    o->preconditioner = 0;
    o->field_cg = 0;
}

mag_ctx *mag_create(const mag_options *opt)
{
    mag_ctx *ctx = new (std::nothrow) mag_ctx();
    if (!ctx) return nullptr;
    if (opt)
        ctx->opt = *opt;
    else
        mag_default_options(&ctx->opt);
    mag_options &o = ctx->opt;
    if (o.tile_nodes != 256 && o.tile_nodes != 512 && o.tile_nodes != 1024) o.tile_nodes = 0; // 0 = automatic
    if (o.preconditioner < 0 || o.preconditioner > 2) o.preconditioner = 0;
    if (o.field_cg < 0 || o.field_cg > 3) o.field_cg = 0;
    if (o.check_every < 2) o.check_every = 2;
    if (o.check_every & 1) ++o.check_every; // p ping-pong parity must restart at 0 every block
    if (o.check_every > 4096) o.check_every = 4096;
    if (o.max_iter < 0) o.max_iter = 0;
    if (o.history_len < 0) o.history_len = 0;
    if (!(o.tol >= 0.0)) o.tol = MAG_TARGET_CG_COST;
    ctx->B = o.tile_nodes ? o.tile_nodes : 512;
    ctx->device = o.device;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    for (int i = 0; e == hipSuccess && i < 10; ++i) e = hipEventCreate(&ctx->ev[i]);
    for (int i = 0; e == hipSuccess && i < 2; ++i) e = hipEventCreateWithFlags(&ctx->evPoll[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_state, 3 * sizeof(CgState), hipHostMallocDefault);
    if (e == hipSuccess)
        e = hipHostMalloc((void **)&ctx->h_fstate, 3 * sizeof(magk::FusedState), hipHostMallocDefault);
    if (e != hipSuccess) {
        fail(ctx, MAG_ERR_HIP, "no usable HIP device %d: %s (this library has no CPU path)", ctx->device,
             hipGetErrorString(e));
        ctx->hip_ok = false;
    } else {
        ctx->hip_ok = true;
    }
    return ctx;
}

// Inboxes created in THIS process, by their IPC handle: ranks may be threads of one process (one context each, on one
// GPU or several), and HIP does not open an IPC handle in the process that exported it -- such a peer is reached
// through the pointer itself.
static std::mutex g_inbox_mu;
static std::map<std::array<uint8_t, MAG_IPC_HANDLE_BYTES>, void *> g_inbox_here;

static void inbox_release(mag_ctx *ctx)
{
    for (int r = 0; r < 8; ++r) {
        if (ctx->inbox_peer[r] && ctx->inbox_peer[r] != ctx->inbox_own && !ctx->inbox_peer_local[r])
            (void)hipIpcCloseMemHandle(ctx->inbox_peer[r]);
        ctx->inbox_peer[r] = nullptr;
        ctx->inbox_peer_local[r] = false;
    }
    if (ctx->inbox_own) {
        std::lock_guard<std::mutex> lk(g_inbox_mu);
        g_inbox_here.erase(ctx->inbox_handle);
    }
    if (ctx->inbox_own) (void)hipFree(ctx->inbox_own);
    ctx->inbox_own = nullptr;
    ctx->inbox_bytes = 0;
    ctx->inbox_ready = false;
}

void mag_destroy(mag_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->hip_ok) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        ctx->comm.destroy();
        if (ctx->win_host) (void)hipHostUnregister(ctx->win_host);
        inbox_release(ctx);
        if (ctx->graph) (void)hipGraphExecDestroy(ctx->graph);
        if (ctx->h_state) (void)hipHostFree(ctx->h_state);
        if (ctx->h_fstate) (void)hipHostFree(ctx->h_fstate);
        for (int i = 0; i < 10; ++i)
            if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
        for (int i = 0; i < 7; ++i)
            if (ctx->evV[i]) (void)hipEventDestroy(ctx->evV[i]);
        for (int i = 0; i < 2; ++i)
            if (ctx->evPoll[i]) (void)hipEventDestroy(ctx->evPoll[i]);
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

const char *mag_last_error(const mag_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

double mag_compute_element_area(const double *xy, const int32_t *tri)
{
    // solver.rs:187-193, signed
    const double x0 = xy[2 * tri[0]], y0 = xy[2 * tri[0] + 1];
    const double x1 = xy[2 * tri[1]], y1 = xy[2 * tri[1] + 1];
    const double x2 = xy[2 * tri[2]], y2 = xy[2 * tri[2] + 1];
    return 0.5 * (x0 * (y1 - y2) + x1 * (y2 - y0) + x2 * (y0 - y1));
}

void mag_compute_strain_displacement_matrix(const double *xy, const int32_t *tri, double element_area, double *B)
{
    // solver.rs:204-230 (host-side twin of exact.hip:strain_displacement)
    const double x0 = xy[2 * tri[0]], y0 = xy[2 * tri[0] + 1];
    const double x1 = xy[2 * tri[1]], y1 = xy[2 * tri[1] + 1];
    const double x2 = xy[2 * tri[2]], y2 = xy[2 * tri[2] + 1];
    const double b1 = y1 - y2, b2 = y2 - y0, b3 = y0 - y1;
    const double g1 = x2 - x1, g2 = x0 - x2, g3 = x1 - x0;
    const double m[18] = {b1, 0., b2, 0., b3, 0., 0., g1, 0., g2, 0., g3, g1, b1, g2, b2, g3, b3};
    const double d = 2.0 * element_area;
    for (int i = 0; i < 18; ++i) B[i] = m[i] / d;
}

void mag_compute_stress_strain_matrix(double poisson_ratio, double youngs_modulus, double *D)
{
    // solver.rs:240-250
    const double nu = poisson_ratio;
    const double m[9] = {1.0, nu, 0.0, nu, 1.0, 0.0, 0.0, 0.0, (1.0 - nu) / 2.0};
    const double s = youngs_modulus / (1.0 - nu * nu);
    for (int i = 0; i < 9; ++i) D[i] = m[i] * s;
}

namespace {

// solver.rs:365-404,427-432: the right-hand side of one set of prescribed values, Hilbert numbering.  from_order: the ordering
// phase has written b = 0.0 + f for every node from THIS f_in (apply_order); a load case's f was not there then and gets the
// same values from rhs_untouched.  Then only the rows with a prescribed column need K, and the pattern kernel has flagged them
// (bc_touch_ready); otherwise the full pass
int rhs_phase(mag_ctx *ctx, const double *u_in, const double *f_in, double *bP, bool from_order)
{
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N;
    if (wants_csr(ctx)) {
        HIPCHK(ctx->bc_touch.reserve((size_t)N + 16));
        if (ctx->bc_touch_ready) {
            if (!from_order) magk::rhs_untouched(ctx->uknown.as<uint8_t>(), f_in, ctx->perm.as<uint32_t>(), N, bP, s);
            magk::rhs_touched(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), ctx->kval.as<double>(),
                              ctx->uknown.as<uint8_t>(), u_in, f_in, ctx->perm.as<uint32_t>(), ctx->bc_touch.as<uint8_t>(), N, bP, s);
        } else {
            magk::rhs_from_csr(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), ctx->kval.as<double>(),
                               ctx->uknown.as<uint8_t>(), u_in, f_in, ctx->perm.as<uint32_t>(), ctx->bc_touch.as<uint8_t>(),
                               ctx->bc_touch_ready, N, bP, s);
        }
    } else {
        magk::known_to_hilbert(u_in, ctx->uknown.as<uint8_t>(), ctx->iperm.as<int32_t>(), N, ctx->tmpP.as<double>(), s);
        if (int rc = apply_plain(ctx, ctx->tmpP.as<double>(), ctx->q.as<double>(), 0)) return rc;
        magk::rhs_from_apply(ctx->q.as<double>(), f_in, ctx->uknown.as<uint8_t>(), ctx->perm.as<uint32_t>(), N, bP, s);
    }
    return MAG_OK;
}

// solver.rs:435-441 for the right-hand side in ctx->bP: the CG phase the options and the mesh select, and argmin's best_param
// at the iteration cap.  Fills the solve's part of ctx->stats; the solution is in ctx->x (ctx->u with the CSR operator).
int cg_solve(mag_ctx *ctx)
{
    mag_stats &st = ctx->stats;
    const bool csr_op = ctx->opt.cg_operator == MAG_OP_CSR;
    const bool f32 = ctx->opt.precision == 1;
    if (ctx->opt.preconditioner != 0 && (csr_op || f32 || !ctx->fused))
        return fail(ctx, MAG_ERR_BAD_ARGS,
                    "preconditioner needs the fused LDS iteration: cg_variant 1, precision fp64, matrix-free operator, "
                    "every tile within LDS");
    const bool field_rows = csr_op && field_cg_selected(ctx); // (mag_options.field_cg: K's block rows, fused)
    ctx->cg_kernel = field_rows ? 5 : (csr_op ? 3 : (f32 ? 4 : (ctx->fused ? 1 : 0)));
    ctx->exchange_kind = ctx->dist ? 1 : 0; // the phases that trade through the inboxes say so themselves
    ctx->persist_timed_out = false;
    ctx->exchange_timed_out = false;
    auto cg_dispatch = [&]() {
        if (field_rows && !ctx->fc_ready) return fail(ctx, MAG_ERR_STATE, "field_cg: no block-row table (K has not been assembled under this field)");
        return field_rows ? cg_phase_field(ctx, field_system(ctx))
               : csr_op   ? cg_phase_csr(ctx)
                      : (f32 ? cg_phase_fused32(ctx)
                             : (ctx->persist ? cg_phase_persist(ctx) : (ctx->fused ? cg_phase_fused(ctx) : cg_phase(ctx))));
    };
    if (int rc = cg_dispatch()) return rc;
    st.best_iteration = st.iterations;
    st.termination = st.breakdown ? MAG_TERM_BREAKDOWN : (st.converged ? MAG_TERM_TARGET_COST : MAG_TERM_MAX_ITERS);
    if (st.termination == MAG_TERM_MAX_ITERS && ctx->best_iter >= 1 && ctx->best_iter < st.iterations) {
        // solver.rs:167-174 returns state.best_param: at the iteration cap that is the lowest-cost iterate, not the
        // last one (plain CG's residual norm is not monotone).  The kernels are bitwise reproducible, so the solve is
        // simply repeated up to that iteration -- nothing is paid for this on the hot path.
        const mag_stats first = st;
        const double best_cost = ctx->best_cost;
        const long long best_iter = ctx->best_iter;
        const int64_t cap = ctx->opt.max_iter;
        const int kernel1 = ctx->cg_kernel, exchange1 = ctx->exchange_kind;
        ctx->opt.max_iter = best_iter;
        const int rc = cg_dispatch();
        ctx->opt.max_iter = cap;
        if (rc) return rc;
        // The repeat stands for the first pass only if it WAS the first pass: same kernel, same exchange (a time-out in
        // either pass changes the path and with it the summation orders), and the cost it reports at best_iter is the
        // recorded best cost, bit for bit.  Otherwise the caller is told and gets the cost of what is actually returned.
        const bool same = ctx->cg_kernel == kernel1 && ctx->exchange_kind == exchange1 && st.iterations == best_iter &&
                          memcmp(&st.final_cost, &best_cost, sizeof(double)) == 0;
        const double cost2 = st.final_cost;
        st.iterations = first.iterations; // what argmin's observer prints: state.get_iter() (solver.rs:101-104)
        st.converged = 0;
        st.breakdown = 0;
        st.termination = MAG_TERM_MAX_ITERS;
        st.best_iteration = best_iter;
        st.final_cost = same ? best_cost : cost2;
        st.best_param_mismatch = same ? 0 : 1;
    }
    return MAG_OK;
}

// solver.rs:443-535 for one solution: scatter-back, reactions, stress (caller numbering)
int post_phase(mag_ctx *ctx, const double *xP, const double *u_in, const double *f_in, double *u, double *f, double *stress)
{
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N;
    if (!solution_expanded(ctx)) // (the CSR operator's phase has expanded its solution into u itself)
        magk::scatter_back(xP, ctx->perm.as<uint32_t>(), ctx->uknown.as<uint8_t>(), u_in, N, u, s);
    if (wants_csr(ctx)) {
        magk::reactions_from_csr(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), ctx->kval.as<double>(),
                                 ctx->uknown.as<uint8_t>(), u, f_in, N, f, s);
    } else {
        magk::to_hilbert(u, ctx->iperm.as<int32_t>(), ctx->uknown.as<uint8_t>(), 0, N, ctx->tmpP.as<double>(), s);
        if (int rc = apply_plain(ctx, ctx->tmpP.as<double>(), ctx->q.as<double>(), 0)) return rc;
        magk::reactions_from_apply(ctx->q.as<double>(), ctx->iperm.as<int32_t>(), ctx->uknown.as<uint8_t>(), f_in, N, f, s);
    }
    magk::element_stress(ctx->xy.as<double>(), ctx->conn.as<int32_t>(), u, ctx->E, ctx->nu, ctx->youngs, stress, s);
    return MAG_OK;
}

// the derived results of set `slot` -- sensitivities, adjoint, objective -- go with the solutions they were derived from
void drop_derived(mag_ctx *ctx, int32_t slot)
{
    for (DerivedSet (&pass)[3] : ctx->derived) pass[slot].have = false;
}

// what every run starts with (mag_run, and a set's run): it redoes the whole path -- nothing of a previous run is reused except
// allocations, the single-case results of the context are gone
void begin_run(mag_ctx *ctx)
{
    ctx->stats = {};
    // (under an element stiffness field the order, the tables and the pattern of the field's first run are kept: a design
    // iteration changes the values of K only)
    ctx->have_order = ctx->field_on && ctx->field_sym && ctx->have_order;
    ctx->field_sym = ctx->have_order;
    ctx->have_csr = ctx->have_run = false;
    ctx->fc_build_ms = 0.0;
    drop_derived(ctx, MAG_SET_RUN); // (the single-case results go with every run, a set's included)
    // a context whose on-chip kernel once found the GPU shared is not condemned to stream for ever: after a number of
    // streamed solves (8, doubling per failure) it tries again -- at worst one more spin budget (~0.3 s).  Across ranks
    // the failures are agreed on collectively, so every rank counts the same and retries in the same solve.
    if (ctx->persist_failed && --ctx->persist_retry_in <= 0) ctx->persist_failed = false;
    if (ctx->opt.verbose) printf("info: building element stiffness matrices...\n");
}

} // namespace

int mag_upload(mag_ctx *ctx, const mag_problem *p)
{
    if (ctx && p)
        if (int rc = memory_refused(ctx, p->memory, "mag_upload")) return rc;
    if (int rc = enter(ctx)) return rc;
    if (!p || !p->xy || !p->conn || !p->u_known || !p->u_in || !p->f_in)
        return fail(ctx, MAG_ERR_BAD_ARGS, "null problem pointer");
    const int64_t N = p->num_nodes, E = p->num_elements;
    if (N < 1 || E < 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "empty mesh (nodes=%lld elements=%lld)", (long long)N, (long long)E);
    if (N >= (int64_t(1) << 30) || 9 * E >= (int64_t(1) << 31))
        return fail(ctx, MAG_ERR_TOO_LARGE, "mesh too large for int32 indexing (nodes=%lld elements=%lld)", (long long)N,
                    (long long)E);
    if (!(p->poisson_ratio * p->poisson_ratio != 1.0))
        return fail(ctx, MAG_ERR_BAD_ARGS, "poisson_ratio^2 == 1");
    const hipMemcpyKind kind = p->memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx->xy.reserve(16 * (size_t)N));
    HIPCHK(ctx->conn.reserve(12 * (size_t)E));
    HIPCHK(ctx->uknown.reserve(2 * (size_t)N));
    HIPCHK(ctx->uin.reserve(16 * (size_t)N));
    HIPCHK(ctx->fin.reserve(16 * (size_t)N));
    HIPCHK(hipMemcpyAsync(ctx->xy.p, p->xy, 16 * (size_t)N, kind, s));
    HIPCHK(hipMemcpyAsync(ctx->conn.p, p->conn, 12 * (size_t)E, kind, s));
    HIPCHK(hipMemcpyAsync(ctx->uknown.p, p->u_known, 2 * (size_t)N, kind, s));
    HIPCHK(hipMemcpyAsync(ctx->uin.p, p->u_in, 16 * (size_t)N, kind, s));
    HIPCHK(hipMemcpyAsync(ctx->fin.p, p->f_in, 16 * (size_t)N, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    ctx->N = N;
    ctx->E = E;
    ctx->youngs = p->youngs_modulus;
    ctx->nu = p->poisson_ratio;
    ctx->thick = p->part_thickness;
    ctx->have_problem = true;
    ctx->have_order = ctx->have_csr = ctx->have_run = false;
    ctx->field_on = ctx->field_sym = ctx->design_on = false; // the field and the design belong to the mesh they were given for
    ctx->sens_tab_ready = false;
    ctx->cases.reset();
    ctx->variants.reset();
    ctx->modal.reset();
    ctx->buckling.reset();
    ctx->tr_have = false;
    ctx->nt_have = false;
    ctx->tt_have = false;
    ctx->rf_have = false;
    for (int32_t slot = MAG_SET_RUN; slot <= MAG_SET_VARIANTS; ++slot) drop_derived(ctx, slot);
    return MAG_OK;
}

int mag_run(mag_ctx *ctx)
{
    if (int rc = enter(ctx)) return rc;
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "mag_run before mag_upload");
    if (ctx->field_on)
        if (int rc = field_context_refused(ctx, "mag_run")) return rc;
    FieldOperator field_op(ctx);
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N, E = ctx->E;
    mag_stats &st = ctx->stats;
    begin_run(ctx);
    const bool kept_sym = ctx->field_sym; // the order and the pattern are those of an earlier run under this field

    HIPCHK(hipEventRecord(ctx->ev[0], s));
    ctx->order_allow_shard = true; // (every rank of the communicator is in mag_run: the sharded phase's all-reduces are safe)
    const int rc_order = ensure_order(ctx);
    ctx->order_allow_shard = false;
    if (rc_order) return rc_order;
    HIPCHK(hipEventRecord(ctx->ev[1], s));
    if (int rc = reserve_cg(ctx)) return rc;
    const bool csr = wants_csr(ctx);
    if (csr) {
        if (!kept_sym)
            if (int rc = csr_symbolic(ctx)) return rc;
        ctx->field_sym = ctx->field_on;
        if (int rc = ensure_field_table(ctx)) return rc; // (mag_options.field_cg: built once, kept like the pattern)
        HIPCHK(hipEventRecord(ctx->ev[2], s)); // (K_e is evaluated inside the row assembly: ms_element is 0 and no event pair is
                                               // spent on it -- an empty pair still costs ~5 us of stream time)
        if (ctx->opt.verbose) printf("info: building total stiffness matrix...\n");
        if (int rc = gather_phase(ctx)) return rc;
        ctx->have_csr = true;
        HIPCHK(hipEventRecord(ctx->ev[4], s));
        if (ctx->opt.verbose) printf("info: setting up system...\n");
    } else {
        HIPCHK(hipEventRecord(ctx->ev[2], s));
        HIPCHK(hipEventRecord(ctx->ev[4], s));
    }
    // (a kept order has not written b = 0.0 + f in this run: rhs_untouched writes the same values)
    if (int rc = rhs_phase(ctx, ctx->uin.as<double>(), ctx->fin.as<double>(), ctx->bP.as<double>(), ctx->b_from_order && !kept_sym)) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[5], s));

    if (ctx->opt.verbose) printf("info: solving...\n");
    HIPCHK(ctx->u.reserve(16 * (size_t)N));
    HIPCHK(ctx->f.reserve(16 * (size_t)N));
    HIPCHK(ctx->stress.reserve(8 * (size_t)E));
    if (int rc = cg_solve(ctx)) return rc;
    HIPCHK(hipEventRecord(ctx->ev[6], s));
    if (ctx->opt.verbose)
        printf("info: finished conjugate gradient approximation in %lld iterations\n", (long long)st.iterations);

    if (int rc = post_phase(ctx, ctx->x.as<double>(), ctx->uin.as<double>(), ctx->fin.as<double>(), ctx->u.as<double>(),
                            ctx->f.as<double>(), ctx->stress.as<double>()))
        return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[7], s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->opt.verbose) printf("info: solve complete\n");

    st.ms_order = kept_sym ? 0.0 : ev_ms(ctx->ev[0], ctx->ev[1]); // (kept: neither phase ran)
    st.ms_csr_symbolic = kept_sym ? ctx->fc_build_ms : ev_ms(ctx->ev[1], ctx->ev[2]); // (kept: at most the block-row table)
    st.ms_element = 0.0; // part of ms_assemble (the assembly kernels evaluate the elements on the fly)
    st.ms_assemble = ev_ms(ctx->ev[2], ctx->ev[4]);
    st.ms_bc = ev_ms(ctx->ev[4], ctx->ev[5]);
    st.ms_cg = ev_ms(ctx->ev[5], ctx->ev[6]);
    st.ms_post = ev_ms(ctx->ev[6], ctx->ev[7]);
    st.ms_total = ev_ms(ctx->ev[0], ctx->ev[7]);
    st.nnz = csr ? 4 * ctx->nb : 0;
    st.num_tiles = ctx->T;
    st.ell_entries = ctx->ell_total;
    st.halo_nodes = ctx->halo_total;
    st.max_tile_halo = ctx->max_halo;
    st.lds_operator = ctx->use_lds ? 1 : 0;
    st.cg_kernel = ctx->cg_kernel;
    st.exchange = ctx->exchange_kind;
    st.n_free = ctx->nf;
    ctx->have_run = true;
    st.persist_timeout = ctx->persist_timed_out ? 1 : 0;
    st.edge_blocks = ctx->cg_kernel == 2 ? ctx->edge_blocks : 0;
    st.tiles_per_workgroup = ctx->cg_kernel == 2 ? ctx->persist_k : 0;
    st.exchange_timeout = ctx->exchange_timed_out ? 1 : 0;
    if (st.breakdown)
        return fail(ctx, MAG_ERR_NOT_CONVERGED, "Conjugate Gradient error: non-finite residual after %lld iterations",
                    (long long)st.iterations);
    // The iteration cap is a NORMAL termination in the reference (argmin's MaxItersReached; solver.rs:149-176 returns
    // Ok(best_param)): MAG_OK, stats.converged = 0, stats.termination = MAG_TERM_MAX_ITERS, the best iterate returned.
    if (!st.converged)
        ctx->err = "Conjugate Gradient stopped at the iteration cap (" + std::to_string((long long)st.iterations) +
                   " iterations) above the target cost: best iterate returned (cost " + std::to_string(st.final_cost) + ")";
    return MAG_OK;
}

int mag_download(mag_ctx *ctx, mag_result *r)
{
    if (ctx && r)
        if (int rc = memory_refused(ctx, r->memory, "mag_download")) return rc;
    if (int rc = enter(ctx)) return rc;
    if (!r) return fail(ctx, MAG_ERR_BAD_ARGS, "null result");
    if (!ctx->have_run) return fail(ctx, MAG_ERR_STATE, "mag_download before a completed mag_run");
    const hipMemcpyKind kind = r->memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipStream_t s = ctx->stream;
    if (r->u_out) HIPCHK(hipMemcpyAsync(r->u_out, ctx->u.p, 16 * (size_t)ctx->N, kind, s));
    if (r->f_out) HIPCHK(hipMemcpyAsync(r->f_out, ctx->f.p, 16 * (size_t)ctx->N, kind, s));
    if (r->stress_out) HIPCHK(hipMemcpyAsync(r->stress_out, ctx->stress.p, 8 * (size_t)ctx->E, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// ---- load cases: num_cases sets of prescribed values on the uploaded mesh (same mesh, material and u_known mask) ----
int mag_set_load_cases(mag_ctx *ctx, int32_t num_cases, const double *u_in, const double *f_in, int32_t memory)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (num_cases < 1) return fail(ctx, MAG_ERR_BAD_ARGS, "num_cases = %d: at least one load case", (int)num_cases);
    if (!u_in || !f_in) return fail(ctx, MAG_ERR_BAD_ARGS, "null load-case pointer");
    if (int rc = memory_refused(ctx, memory, "mag_set_load_cases")) return rc;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "load cases run on one GPU: this context has a communicator of %d ranks", ctx->comm.nranks);
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "mag_set_load_cases before mag_upload");
    if (int rc = enter(ctx)) return rc;
    ctx->cases.have = ctx->cases.have_run = false;
    drop_derived(ctx, MAG_SET_CASES);
    const size_t bytes = 16 * (size_t)ctx->N * (size_t)num_cases;
    const hipMemcpyKind kind = memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx->cases.uin.reserve(bytes));
    HIPCHK(ctx->cases.fin.reserve(bytes));
    HIPCHK(hipMemcpyAsync(ctx->cases.uin.p, u_in, bytes, kind, s));
    HIPCHK(hipMemcpyAsync(ctx->cases.fin.p, f_in, bytes, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    ctx->cases.count = num_cases;
    ctx->cases.have = true;
    return MAG_OK;
}

namespace {

// The uploaded problem is lent to a member that runs through the single-case phases and comes back: the context's u_in / f_in
// (mag_upload's) take the member's values; with `whole` (design variants) its coordinates and material go into the context too.
// keep = the uploaded u_in, f_in and -- whole -- xy
struct LentProblem {
    mag_ctx *ctx;
    DevBuf &keep;
    const bool whole;
    const size_t bytes; // of one of the vectors
    const double youngs, nu, thick;
    bool armed = false;
    LentProblem(mag_ctx *c, DevBuf &k, bool w)
        : ctx(c), keep(k), whole(w), bytes(16 * (size_t)c->N), youngs(c->youngs), nu(c->nu), thick(c->thick)
    {
    }
    int lend() // before the first member that runs alone
    {
        if (armed) return MAG_OK;
        hipStream_t s = ctx->stream;
        HIPCHK(keep.reserve((whole ? 3 : 2) * bytes));
        if (whole) HIPCHK(hipMemcpyAsync(keep.as<char>() + 2 * bytes, ctx->xy.p, bytes, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(keep.p, ctx->uin.p, bytes, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(keep.as<char>() + bytes, ctx->fin.p, bytes, hipMemcpyDeviceToDevice, s));
        armed = true;
        return MAG_OK;
    }
    // the uploaded vectors while they are lent (nullptr: they are still in the context)
    const double *uin() const { return armed ? keep.as<double>() : nullptr; }
    const double *fin() const { return armed ? (const double *)(keep.as<char>() + bytes) : nullptr; }
    const double *xy() const { return armed && whole ? (const double *)(keep.as<char>() + 2 * bytes) : nullptr; }
    ~LentProblem()
    {
        if (!armed) return;
        hipStream_t s = ctx->stream;
        if (whole) (void)hipMemcpyAsync(ctx->xy.p, keep.as<char>() + 2 * bytes, bytes, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(ctx->uin.p, keep.p, bytes, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(ctx->fin.p, keep.as<char>() + bytes, bytes, hipMemcpyDeviceToDevice, s);
        (void)hipStreamSynchronize(s);
        if (!whole) return;
        ctx->youngs = youngs;
        ctx->nu = nu;
        ctx->thick = thick;
    }
};

// cg_solve for the right-hand side in ctx->bP as member c of a set (a load case, a design variant): history_len and verbose are
// member 0's; `out` gets the solve's statistics (the stream is idle afterwards)
int cg_solve_member(mag_ctx *ctx, int32_t c, mag_stats &out, bool timed_out_before)
{
    hipStream_t s = ctx->stream;
    const int32_t hist_len = ctx->opt.history_len, verbose = ctx->opt.verbose;
    if (c != 0) ctx->opt.history_len = ctx->opt.verbose = 0;
    ctx->stats = {};
    HIPCHK(hipEventRecord(ctx->ev[8], s));
    const int rc = cg_solve(ctx);
    ctx->opt.history_len = hist_len;
    ctx->opt.verbose = verbose;
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->ev[9], s));
    HIPCHK(hipStreamSynchronize(s));
    out = ctx->stats;
    out.ms_cg = ev_ms(ctx->ev[8], ctx->ev[9]);
    out.cg_kernel = ctx->cg_kernel;
    out.exchange = ctx->exchange_kind;
    out.persist_timeout = (timed_out_before || ctx->persist_timed_out) ? 1 : 0;
    out.edge_blocks = ctx->cg_kernel == 2 ? ctx->edge_blocks : 0;
    out.tiles_per_workgroup = ctx->cg_kernel == 2 ? ctx->persist_k : 0;
    return MAG_OK;
}

// one case through the single-case CG phases (cg_solve: the phase the options select, its time-out fall-back, best_param):
// its loads and right-hand side into the context's buffers, its solution out of them.
int solve_case_alone(mag_ctx *ctx, MemberSet &set, int32_t c, mag_stats &out, bool timed_out_before)
{
    hipStream_t s = ctx->stream;
    const size_t vb = 16 * (size_t)ctx->N;
    HIPCHK(hipMemcpyAsync(ctx->uin.p, set.uin.as<char>() + vb * c, vb, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->fin.p, set.fin.as<char>() + vb * c, vb, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bP.p, set.bP.as<char>() + vb * c, vb, hipMemcpyDeviceToDevice, s));
    if (int rc = cg_solve_member(ctx, c, out, timed_out_before)) return rc;
    if (solution_expanded(ctx))
        HIPCHK(hipMemcpyAsync(set.u.as<char>() + vb * c, ctx->u.p, vb, hipMemcpyDeviceToDevice, s));
    else
        HIPCHK(hipMemcpyAsync(set.x.as<char>() + vb * c, ctx->x.p, vb, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// ONE launch of the load-case kernel (or of its design-variant form) for members [c0, c0 + n) of a set: P carries the members'
// bP and x and what they share; their granules, records, timeout words and states are the context's launch buffers.  Afterwards
// every member's CG statistics are in stats[c0 + k]; a member whose group gave up at its barrier (timed_out) or that stopped at
// the iteration cap with an earlier best iterate is marked `alone`: the caller redoes it through the single-case phases.
int launch_members(mag_ctx *ctx, magk::PersistParams &P, int32_t G, int32_t c0, int32_t n, int eb_mode, std::vector<mag_stats> &stats,
                   std::vector<uint8_t> &alone, std::vector<uint8_t> &timed_out, magk::PersistMembers members)
{
    using magk::FusedState;
    hipStream_t s = ctx->stream;
    const size_t qg_bytes = 2 * 32 * (size_t)ctx->N, rec_bytes = 2 * 64 * (size_t)G;
    HIPCHK(ctx->launch_qx.reserve(qg_bytes * n));
    HIPCHK(ctx->launch_part.reserve(rec_bytes * n));
    HIPCHK(ctx->launch_sync.reserve(64 * (size_t)n));
    HIPCHK(ctx->launch_state.reserve(sizeof(FusedState) * (size_t)n));
    std::vector<FusedState> h_st((size_t)n);
    std::vector<uint32_t> h_sync(16 * (size_t)n);
    // tags of a previous launch must not look current: zeroed before EVERY launch, as cg_phase_persist does
    HIPCHK(hipMemsetAsync(ctx->launch_qx.p, 0, qg_bytes * n, s));
    HIPCHK(hipMemsetAsync(ctx->launch_part.p, 0, rec_bytes * n, s));
    HIPCHK(hipMemsetAsync(ctx->launch_sync.p, 0, 64 * (size_t)n, s));
    HIPCHK(hipMemsetAsync(ctx->launch_state.p, 0, sizeof(FusedState) * (size_t)n, s));
    P.qg = ctx->launch_qx.as<unsigned long long>();
    P.recg = ctx->launch_part.as<unsigned long long>();
    P.sync = ctx->launch_sync.as<uint32_t>();
    P.st = ctx->launch_state.as<FusedState>();
    P.hist_len = c0 == 0 ? ctx->opt.history_len : 0; // (member 0's alone: the kernel keeps it from the launch's other members)
    HIPCHK(hipEventRecord(ctx->ev[8], s));
    if (!magk::persist_launch(P, ctx->B, G, n, members, eb_mode, s)) // (unreachable: run_members has asked persist_shape)
        return fail(ctx, MAG_ERR_STATE, "on-chip CG: no kernel for this shape");
    HIPCHK(hipEventRecord(ctx->ev[9], s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_st.data(), ctx->launch_state.p, sizeof(FusedState) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_sync.data(), ctx->launch_sync.p, 64 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double ms = ev_ms(ctx->ev[8], ctx->ev[9]);
    for (int32_t k = 0; k < n; ++k) {
        const FusedState &st = h_st[(size_t)k];
        mag_stats &cs = stats[(size_t)(c0 + k)];
        cs.ms_cg = ms;
        if (h_sync[16 * (size_t)k + 9] != 0 || !st.done) { // this member's group gave up at its barrier
            alone[(size_t)(c0 + k)] = timed_out[(size_t)(c0 + k)] = 1;
            continue;
        }
        cs.iterations = st.iterations;
        cs.final_cost = st.final_cost;
        cs.rhs_norm = std::sqrt(st.bb);
        cs.converged = st.converged;
        cs.breakdown = st.breakdown;
        cs.best_iteration = st.iterations;
        cs.termination = st.breakdown ? MAG_TERM_BREAKDOWN : (st.converged ? MAG_TERM_TARGET_COST : MAG_TERM_MAX_ITERS);
        cs.cg_kernel = 2;
        cs.edge_blocks = eb_mode;
        cs.tiles_per_workgroup = ctx->persist_k;
        // the iteration cap with an earlier best iterate: best_param is recovered by the single-case path's repeat
        if (cs.termination == MAG_TERM_MAX_ITERS && st.best_iter >= 1 && st.best_iter < st.iterations) alone[(size_t)(c0 + k)] = 1;
    }
    return MAG_OK;
}

// what every member of a set reports alike: the shared phases' times, the mesh's figures; the status of the first member that
// broke down (`what`: "load case" / "variant")
int finish_member_stats(mag_ctx *ctx, std::vector<mag_stats> &stats, bool csr, const char *what)
{
    int status = MAG_OK;
    for (size_t c = 0; c < stats.size(); ++c) {
        mag_stats &cs = stats[c];
        cs.ms_order = ev_ms(ctx->ev[0], ctx->ev[1]); // the shared phases: the same in every member
        cs.ms_csr_symbolic = ev_ms(ctx->ev[1], ctx->ev[2]);
        cs.ms_total = ev_ms(ctx->ev[0], ctx->ev[7]);
        cs.nnz = csr ? 4 * ctx->nb : 0;
        cs.num_tiles = ctx->T;
        cs.ell_entries = ctx->ell_total;
        cs.halo_nodes = ctx->halo_total;
        cs.max_tile_halo = ctx->max_halo;
        cs.lds_operator = ctx->use_lds ? 1 : 0;
        cs.n_free = ctx->nf;
        if (cs.breakdown && status == MAG_OK)
            status = fail(ctx, MAG_ERR_NOT_CONVERGED, "%s %d: Conjugate Gradient error: non-finite residual after %lld iterations",
                          what, (int)c, (long long)cs.iterations);
    }
    return status;
}

// What differs between the sets when run_members solves them.  after_launch and post may be empty.
struct MemberHooks {
    // after the shared phases (order, tables, CSR pattern; ev[2] is recorded): the set's buffers -- and, for load cases, K and
    // every case's right-hand side
    std::function<int()> prepare;
    // side by side, around ONE launch for members [c0, c0 + n): what the launch reads (P.bP and P.x at the least), what follows it
    std::function<int(magk::PersistParams &P, int32_t c0, int32_t n, int eb_mode)> before_launch;
    std::function<int(int32_t c0, int32_t n)> after_launch;
    // member c through the single-case phases, the uploaded problem lent to it
    std::function<int(int32_t c, mag_stats &out, bool timed_out_before)> solve_alone;
    // after the last solve, before ev[7]
    std::function<int()> post;
    // the set's phase times into a member's statistics (the stream is idle)
    std::function<void(mag_stats &cs)> times;
};

// Solve the members of `set` (its state checks are the caller's): the shared phases once, then the CG solves side by side in
// chunks of floor(CUs / G) members per launch where the on-chip kernel takes them, anything else -- and every member a launch
// could not finish -- alone through the single-case phases with the uploaded problem lent to it (`keep`; keep.whole: every
// member is a problem of its own, so side by side needs its K assembled and the hooks build its blocks).
int run_members(mag_ctx *ctx, MemberSet &set, LentProblem &keep, const MemberHooks &hooks)
{
    if (ctx->field_on)
        if (int rc = field_context_refused(ctx, set.run_fn)) return rc;
    if (int rc = enter(ctx)) return rc;
    FieldOperator field_op(ctx); // (under a field: the CSR operator's phase, hence one member after another)
    hipStream_t s = ctx->stream;
    const int32_t L = set.count;
    set.have_run = false;
    if (!set.adjoint) drop_derived(ctx, set.slot); // (an adjoint set's run leaves the results of the set it differentiates)
    begin_run(ctx);
    set.stats.assign((size_t)L, mag_stats{});
    int32_t *info = set.info;
    info[0] = L;
    info[1] = info[2] = info[3] = 0;

    // ---- once for all members: the Hilbert order OF THE UPLOADED COORDINATES, incidence, tile, ring and halo tables, masks, the
    // CSR pattern, the fan classification -- nothing here reads a prescribed VALUE (apply_order's b = 0.0 + f of the context's
    // own f_in is simply not used)
    HIPCHK(hipEventRecord(ctx->ev[0], s));
    if (int rc = ensure_order(ctx)) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], s));
    if (int rc = reserve_cg(ctx)) return rc;
    const bool csr = wants_csr(ctx);
    const bool kept_sym = ctx->field_sym; // (begin_run: the order and the pattern of an earlier run under this field)
    if (csr && !kept_sym)
        if (int rc = csr_symbolic(ctx)) return rc;
    ctx->field_sym = ctx->field_on && csr;
    if (csr)
        if (int rc = ensure_field_table(ctx)) return rc;
    HIPCHK(hipEventRecord(ctx->ev[2], s));
    if (int rc = hooks.prepare()) return rc;
    if (ctx->opt.verbose) printf("info: solving...\n");

    // ---- CG.  On-chip and at least two members fit the chip: chunks of floor(CUs / G) members per launch, G = the workgroups
    // one member needs, persist_k as the single-case path chose it (more tiles per workgroup would change the summation order).
    // Anything else: one member after another through the single-case phases.
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    const int32_t G = ctx->persist_grid, fit = G >= 1 ? cus / G : 0;
    int32_t per_launch = 0;
    // (an adjoint set is solved as the set it differentiates is: the variants' by the variant kernels, the others as load cases)
    const magk::PersistMembers members = set.slot == MAG_SET_VARIANTS ? magk::PERSIST_VARIANTS : magk::PERSIST_CASES;
    magk::PersistShape shape;
    magk::PersistParams P = {};
    int eb_mode = 0;
    // (ctx->persist: cg_variant 2, fp64, matrix-free, no preconditioner, not in back-off, the mesh fits -- ensure_order)
    if (ctx->persist && (csr || !keep.whole) && ctx->opt.cg_operator != MAG_OP_CSR && ctx->opt.precision == 0 && fit >= 2) {
        P.nranks = 1;
        persist_common_params(ctx, false, P);
        if (int rc = persist_prepare_blocks(ctx, false, P, eb_mode, !keep.whole)) return rc;
        if (magk::persist_shape(ctx->B, 1, G, ctx->persist_k, eb_mode, members, shape)) per_launch = fit;
    }
    info[1] = per_launch;
    std::vector<uint8_t> alone((size_t)L, per_launch ? 0 : 1), timed_out((size_t)L, 0);
    if (per_launch) {
        for (int32_t c0 = 0; c0 < L; c0 += per_launch) {
            const int32_t n = std::min(per_launch, L - c0);
            if (int rc = hooks.before_launch(P, c0, n, eb_mode)) return rc;
            if (int rc = launch_members(ctx, P, G, c0, n, eb_mode, set.stats, alone, timed_out, members)) return rc;
            ++info[2];
            if (hooks.after_launch)
                if (int rc = hooks.after_launch(c0, n)) return rc;
        }
        ctx->cg_kernel = 2;
    }
    bool backed_off = false;
    for (int32_t c = 0; c < L; ++c) {
        if (!alone[(size_t)c]) continue;
        if (timed_out[(size_t)c] && !backed_off) { // the single-case path's bookkeeping: the context streams from here on
            persist_back_off(ctx);
            backed_off = true;
        }
        if (int rc = keep.lend()) return rc;
        if (int rc = hooks.solve_alone(c, set.stats[(size_t)c], timed_out[(size_t)c] != 0)) return rc;
        if (per_launch) ++info[3];
    }
    if (per_launch && !backed_off) ctx->persist_backoff = 0; // co-resident: the next failure starts from the short wait
    if (ctx->opt.verbose)
        printf("info: finished conjugate gradient approximation in %lld iterations\n", (long long)set.stats[0].iterations);
    if (hooks.post)
        if (int rc = hooks.post()) return rc;
    HIPCHK(hipEventRecord(ctx->ev[7], s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->opt.verbose) printf("info: solve complete\n");

    for (mag_stats &cs : set.stats) hooks.times(cs);
    const int status = finish_member_stats(ctx, set.stats, csr, set.noun);
    ctx->stats = set.stats[0];
    set.have_run = true;
    return status;
}

// mag_download_case / mag_download_variant (`fn_name`), and the sets' other getters
int download_member(mag_ctx *ctx, const MemberSet &set, int32_t i, mag_result *r, const char *fn_name)
{
    if (!r) return fail(ctx, MAG_ERR_BAD_ARGS, "null result");
    if (int rc = memory_refused(ctx, r->memory, fn_name)) return rc;
    if (i < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "%s %d out of range", set.noun, (int)i);
    if (!set.have_run) return fail(ctx, MAG_ERR_STATE, "%s before a completed %s", fn_name, set.run_fn);
    if (i >= set.count) return fail(ctx, MAG_ERR_BAD_ARGS, "%s %d out of range [0, %d)", set.noun, (int)i, (int)set.count);
    if (int rc = enter(ctx)) return rc;
    const hipMemcpyKind kind = r->memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipStream_t s = ctx->stream;
    const size_t vb = 16 * (size_t)ctx->N, eb = 8 * (size_t)ctx->E, c = (size_t)i;
    if (r->u_out) HIPCHK(hipMemcpyAsync(r->u_out, set.u.as<char>() + vb * c, vb, kind, s));
    if (r->f_out) HIPCHK(hipMemcpyAsync(r->f_out, set.f.as<char>() + vb * c, vb, kind, s));
    if (r->stress_out) HIPCHK(hipMemcpyAsync(r->stress_out, set.stress.as<char>() + eb * c, eb, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int member_stats(const MemberSet &set, int32_t i, mag_stats *st)
{
    if (!st || i < 0) return MAG_ERR_BAD_ARGS;
    if (!set.have_run) return MAG_ERR_STATE;
    if (i >= set.count) return MAG_ERR_BAD_ARGS;
    *st = set.stats[(size_t)i];
    return MAG_OK;
}

int set_info(const MemberSet &set, int32_t info[4])
{
    if (!info) return MAG_ERR_BAD_ARGS;
    if (!set.have_run) return MAG_ERR_STATE;
    for (int k = 0; k < 4; ++k) info[k] = set.info[k];
    return MAG_OK;
}

// the members of `set` as load cases of the uploaded mesh (mag_run_cases; the adjoint systems of a run or of load cases)
int run_case_set(mag_ctx *ctx, MemberSet &set)
{
    hipStream_t s = ctx->stream;
    const int32_t L = set.count;
    const size_t vb = 16 * (size_t)ctx->N, eb = 8 * (size_t)ctx->E;
    auto at = [](const DevBuf &b, size_t stride, int32_t c) { return (double *)(b.as<char>() + stride * (size_t)c); };
    LentProblem keep(ctx, set.keep, false);
    MemberHooks h;
    h.prepare = [&]() -> int { // K once, then per case the right-hand side: the single-case arithmetic in the single-case order
        if (wants_csr(ctx)) {
            if (ctx->opt.verbose) printf("info: building total stiffness matrix...\n");
            if (int rc = gather_phase(ctx)) return rc;
            ctx->have_csr = true;
        }
        HIPCHK(hipEventRecord(ctx->ev[4], s));
        if (ctx->opt.verbose) printf("info: setting up system...\n");
        HIPCHK(set.bP.reserve(vb * L));
        HIPCHK(set.x.reserve(vb * L));
        HIPCHK(set.u.reserve(vb * L));
        HIPCHK(set.f.reserve(vb * L));
        HIPCHK(set.stress.reserve(eb * L));
        HIPCHK(ctx->u.reserve(vb)); // (the CSR operator's phase expands into the context's u)
        for (int32_t c = 0; c < L; ++c)
            if (int rc = rhs_phase(ctx, at(set.uin, vb, c), at(set.fin, vb, c), at(set.bP, vb, c), false)) return rc;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[5], s));
        return MAG_OK;
    };
    h.before_launch = [&](magk::PersistParams &P, int32_t c0, int32_t, int) -> int {
        P.bP = (const double2 *)at(set.bP, vb, c0);
        P.x = (double2 *)at(set.x, vb, c0);
        return MAG_OK;
    };
    h.solve_alone = [&](int32_t c, mag_stats &out, bool timed_out_before) { return solve_case_alone(ctx, set, c, out, timed_out_before); };
    h.post = [&]() -> int { // per case: scatter-back, reactions, stress
        HIPCHK(hipEventRecord(ctx->ev[6], s));
        for (int32_t c = 0; c < L; ++c)
            if (int rc = post_phase(ctx, at(set.x, vb, c), at(set.uin, vb, c), at(set.fin, vb, c), at(set.u, vb, c), at(set.f, vb, c),
                                    at(set.stress, eb, c)))
                return rc;
        HIPCHK(hipGetLastError());
        return MAG_OK;
    };
    h.times = [&](mag_stats &cs) {
        cs.ms_element = 0.0;
        cs.ms_assemble = ev_ms(ctx->ev[2], ctx->ev[4]);
        cs.ms_bc = ev_ms(ctx->ev[4], ctx->ev[5]); // all cases' right-hand sides / post-processing
        cs.ms_post = ev_ms(ctx->ev[6], ctx->ev[7]);
    };
    return run_members(ctx, set, keep, h);
}

} // namespace

int mag_run_cases(mag_ctx *ctx)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "load cases run on one GPU: this context has a communicator of %d ranks", ctx->comm.nranks);
    if (!ctx->have_problem || !ctx->cases.have) return fail(ctx, MAG_ERR_STATE, "mag_run_cases before mag_set_load_cases");
    return run_case_set(ctx, ctx->cases);
}

int mag_download_case(mag_ctx *ctx, int32_t case_index, mag_result *r)
{
    return ctx ? download_member(ctx, ctx->cases, case_index, r, "mag_download_case") : MAG_ERR_BAD_ARGS;
}

int mag_get_case_stats(const mag_ctx *ctx, int32_t case_index, mag_stats *st)
{
    return ctx ? member_stats(ctx->cases, case_index, st) : MAG_ERR_BAD_ARGS;
}

int mag_get_cases_info(const mag_ctx *ctx, int32_t info[4]) { return ctx ? set_info(ctx->cases, info) : MAG_ERR_BAD_ARGS; }

// ---- design variants: num_variants shapes / materials / value sets of the uploaded mesh (same connectivity and u_known mask) ----
namespace {

const char *material_error(const double *m) // E, nu, thickness: mag_upload's check
{
    return !(m[1] * m[1] != 1.0) ? "poisson_ratio^2 == 1" : nullptr;
}

int variants_refused(mag_ctx *ctx)
{
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "variants run on one GPU: this context has a communicator of %d ranks", ctx->comm.nranks);
    return MAG_OK;
}

} // namespace

int mag_set_variants(mag_ctx *ctx, int32_t num_variants, const double *xy, const double *material, const double *u_in,
                     const double *f_in, int32_t memory)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, "mag_set_variants");
    if (num_variants < 1) return fail(ctx, MAG_ERR_BAD_ARGS, "num_variants = %d: at least one variant", (int)num_variants);
    if ((u_in == nullptr) != (f_in == nullptr)) return fail(ctx, MAG_ERR_BAD_ARGS, "variants: u_in and f_in come together, or both null");
    if (!xy && !material && !u_in)
        return fail(ctx, MAG_ERR_BAD_ARGS, "variants: at least one of xy, material and the value pair must be given");
    if (int rc = memory_refused(ctx, memory, "mag_set_variants")) return rc;
    if (int rc = variants_refused(ctx)) return rc;
    const int32_t V = num_variants;
    std::vector<double> mat(3 * (size_t)V);
    auto check_materials = [&]() -> int {
        for (int32_t v = 0; v < V; ++v)
            if (const char *why = material_error(&mat[3 * (size_t)v]))
                return fail(ctx, MAG_ERR_BAD_ARGS, "variant %d: %s", (int)v, why);
        return MAG_OK;
    };
    if (material && memory != MAG_MEM_DEVICE) { // host values: checked before anything else is looked at
        memcpy(mat.data(), material, 8 * mat.size());
        if (int rc = check_materials()) return rc;
    }
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "mag_set_variants before mag_upload");
    if (int rc = enter(ctx)) return rc;
    const int64_t N = ctx->N, E = ctx->E;
    const size_t bytes = 16 * (size_t)N * (size_t)V;
    const hipMemcpyKind kind = memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipStream_t s = ctx->stream;
    if (material && memory == MAG_MEM_DEVICE) { // device values: read back and checked before the set is touched, so that a
                                                // refused material leaves the variants as they were, as a host one does
        HIPCHK(hipMemcpyAsync(mat.data(), material, 8 * mat.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (int rc = check_materials()) return rc;
    }
    ctx->variants.have = ctx->variants.have_run = false;
    drop_derived(ctx, MAG_SET_VARIANTS);
    if (!material)
        for (int32_t v = 0; v < V; ++v) {
            mat[3 * (size_t)v + 0] = ctx->youngs;
            mat[3 * (size_t)v + 1] = ctx->nu;
            mat[3 * (size_t)v + 2] = ctx->thick;
        }
    // the CG kernels' constants, by set_material's expressions (the same bits as a solve with that material)
    std::vector<double> cmat(3 * (size_t)V);
    for (int32_t v = 0; v < V; ++v) {
        const double youngs = mat[3 * (size_t)v], nu = mat[3 * (size_t)v + 1], thick = mat[3 * (size_t)v + 2];
        cmat[3 * (size_t)v + 0] = youngs * thick / (2.0 * (1.0 - nu * nu));
        cmat[3 * (size_t)v + 1] = nu;
        cmat[3 * (size_t)v + 2] = (1.0 - nu) / 2.0;
    }
    HIPCHK(ctx->v_mat.reserve(8 * mat.size()));
    HIPCHK(ctx->v_cmat.reserve(8 * cmat.size()));
    HIPCHK(hipMemcpyAsync(ctx->v_mat.p, mat.data(), 8 * mat.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->v_cmat.p, cmat.data(), 8 * cmat.size(), hipMemcpyHostToDevice, s));
    if (xy) {
        HIPCHK(ctx->v_xy.reserve(bytes));
        HIPCHK(hipMemcpyAsync(ctx->v_xy.p, xy, bytes, kind, s));
    }
    if (u_in) {
        HIPCHK(ctx->variants.uin.reserve(bytes));
        HIPCHK(ctx->variants.fin.reserve(bytes));
        HIPCHK(hipMemcpyAsync(ctx->variants.uin.p, u_in, bytes, kind, s));
        HIPCHK(hipMemcpyAsync(ctx->variants.fin.p, f_in, bytes, kind, s));
    }
    HIPCHK(hipStreamSynchronize(s)); // (the host vectors and the caller's buffers are done with)
    if (xy) {
        // the shared ring tables walk every node's triangles in the uploaded orientation: one reduction over (variant, element)
        HIPCHK(ctx->v_bad.reserve(8));
        for (int32_t v0 = 0; v0 < V; v0 += 32768) { // (grid.y holds 65535)
            const int32_t n = std::min<int32_t>(32768, V - v0);
            unsigned long long bad = ~0ull;
            magk::variant_orientation(ctx->xy.as<double>(), ctx->v_xy.as<double>() + 2 * (size_t)N * (size_t)v0,
                                      ctx->conn.as<int32_t>(), N, E, n, ctx->v_bad.as<unsigned long long>(), s);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&bad, ctx->v_bad.p, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (bad != ~0ull)
                return fail(ctx, MAG_ERR_BAD_ARGS,
                            "variant %lld, element %lld: the signed area differs in sign from the uploaded mesh's or is zero "
                            "(variants keep the orientation of every element)",
                            (long long)(v0 + (int64_t)(bad / (unsigned long long)E)), (long long)(bad % (unsigned long long)E));
        }
    }
    ctx->v_mat_h = mat;
    ctx->v_have_xy = xy != nullptr;
    ctx->v_have_loads = u_in != nullptr;
    ctx->variants.count = V;
    ctx->variants.have = true;
    return MAG_OK;
}

namespace {

// where variant v's coordinates and values are: its own, or the uploaded ones (kept aside while they are lent)
const double *variant_xy(const mag_ctx *ctx, const LentProblem &keep, int32_t v)
{
    if (ctx->v_have_xy) return ctx->v_xy.as<double>() + 2 * (size_t)ctx->N * (size_t)v;
    return keep.armed ? keep.xy() : ctx->xy.as<double>();
}
// (`set`: the variants, or their adjoint systems, which always bring loads of their own)
const double *variant_loads(const mag_ctx *ctx, const MemberSet &set, const LentProblem &keep, int32_t v, bool forces)
{
    if (set.adjoint || ctx->v_have_loads) return (forces ? set.fin : set.uin).as<double>() + 2 * (size_t)ctx->N * (size_t)v;
    if (keep.armed) return forces ? keep.fin() : keep.uin();
    return (forces ? ctx->fin : ctx->uin).as<double>();
}

// one variant through the single-case phases, the shared tables kept: its coordinates (permuted into xyP and the tiles' halo
// copies), material and values into the context, then K, right-hand side, cg_solve (its time-out fall-back, its best_param
// repeat) and post as mag_run runs them.  The caller has armed `keep`.
int solve_variant_alone(mag_ctx *ctx, MemberSet &set, const LentProblem &keep, int32_t v, mag_stats &out, bool timed_out_before)
{
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N, E = ctx->E;
    const size_t vb = 16 * (size_t)N, eb = 8 * (size_t)E;
    HIPCHK(hipMemcpyAsync(ctx->xy.p, variant_xy(ctx, keep, v), vb, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->uin.p, variant_loads(ctx, set, keep, v, false), vb, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->fin.p, variant_loads(ctx, set, keep, v, true), vb, hipMemcpyDeviceToDevice, s));
    ctx->youngs = ctx->v_mat_h[3 * (size_t)v + 0];
    ctx->nu = ctx->v_mat_h[3 * (size_t)v + 1];
    ctx->thick = ctx->v_mat_h[3 * (size_t)v + 2];
    magk::VariantBatch one = {};
    one.count = 1;
    one.halo = ctx->halo_total;
    magk::variant_coords(ctx->xy.as<double>(), ctx->perm.as<uint32_t>(), ctx->halo_g.as<int32_t>(), N,
                         ctx->use_lds ? ctx->halo_total : 0, one, ctx->xyP.as<double>(), ctx->halo_xy.as<double>(), s);
    if (wants_csr(ctx)) {
        if (int rc = gather_phase(ctx)) return rc;
        ctx->have_csr = true;
    }
    if (int rc = rhs_phase(ctx, ctx->uin.as<double>(), ctx->fin.as<double>(), ctx->bP.as<double>(), false)) return rc;
    HIPCHK(hipGetLastError());
    if (int rc = cg_solve_member(ctx, v, out, timed_out_before)) return rc;
    if (solution_expanded(ctx)) // (that operator's phase has expanded its solution into the context's u)
        HIPCHK(hipMemcpyAsync(set.u.as<char>() + vb * (size_t)v, ctx->u.p, vb, hipMemcpyDeviceToDevice, s));
    if (int rc = post_phase(ctx, ctx->x.as<double>(), ctx->uin.as<double>(), ctx->fin.as<double>(), set.u.as<double>() + 2 * (size_t)N * v,
                            set.f.as<double>() + 2 * (size_t)N * v, (double *)(set.stress.as<char>() + eb * (size_t)v)))
        return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// the members of `set` as design variants of the uploaded mesh: the coordinates and materials of mag_set_variants, the loads
// of `set` (mag_run_variants; the variants' adjoint systems)
int run_variant_set(mag_ctx *ctx, MemberSet &set)
{
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N, E = ctx->E;
    const int32_t V = set.count;
    const size_t vb = 16 * (size_t)N, eb = 8 * (size_t)E;
    LentProblem keep(ctx, set.keep, true);
    // one chunk's members, from before_launch to after_launch
    magk::VariantBatch vbat = {};
    const double *xy = nullptr, *uin = nullptr, *fin = nullptr;
    double *xP = nullptr;
    double ms_phase[6] = {0, 0, 0, 0, 0, 0}; // permute, assemble, right-hand sides, blocks, launches, post: all chunks
    MemberHooks h;
    h.prepare = [&]() -> int {
        for (hipEvent_t &e : ctx->evV)
            if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(set.bP.reserve(vb * V));
        HIPCHK(set.x.reserve(vb * V));
        HIPCHK(set.u.reserve(vb * V));
        HIPCHK(set.f.reserve(vb * V));
        HIPCHK(set.stress.reserve(eb * V));
        HIPCHK(ctx->u.reserve(vb));
        HIPCHK(ctx->f.reserve(vb));
        HIPCHK(ctx->stress.reserve(eb));
        return MAG_OK;
    };
    // a chunk's coordinates, K, right-hand sides and blocks (the first chunk is the largest: its reservations hold for all)
    h.before_launch = [&](magk::PersistParams &P, int32_t c0, int32_t n, int eb_mode) -> int {
        const int64_t npad = (int64_t)ctx->T * ctx->B, halo = std::max<int64_t>(ctx->halo_total, 1);
        const int64_t kb_words = 3 * (int64_t)magk::persist_block_entries() * npad, ovf_words = 4 * (int64_t)std::max(ctx->ovf_total, 1);
        HIPCHK(ctx->v_xyP.reserve(vb * n));
        HIPCHK(ctx->v_halo.reserve(16 * (size_t)halo * n));
        HIPCHK(ctx->v_kval.reserve(8 * 4 * (size_t)ctx->nb * n));
        if (eb_mode) HIPCHK(ctx->v_kblocks.reserve(8 * (size_t)kb_words * n));
        if (eb_mode == 2) HIPCHK(ctx->v_ovf.reserve(8 * (size_t)ovf_words * n));
        vbat = {};
        vbat.count = n;
        vbat.mat = ctx->v_mat.as<double>() + 3 * (size_t)c0;
        vbat.xy = ctx->v_have_xy ? 2 * N : 0;
        vbat.loads = set.adjoint || ctx->v_have_loads ? 2 * N : 0;
        vbat.halo = halo;
        vbat.kval = 4 * ctx->nb;
        xy = variant_xy(ctx, keep, c0);
        uin = variant_loads(ctx, set, keep, c0, false);
        fin = variant_loads(ctx, set, keep, c0, true);
        double *bP = set.bP.as<double>() + 2 * (size_t)N * c0;
        xP = set.x.as<double>() + 2 * (size_t)N * c0;
        HIPCHK(hipEventRecord(ctx->evV[0], s));
        magk::variant_coords(xy, ctx->perm.as<uint32_t>(), ctx->halo_g.as<int32_t>(), N, ctx->halo_total, vbat, ctx->v_xyP.as<double>(),
                             ctx->v_halo.as<double>(), s);
        HIPCHK(hipEventRecord(ctx->evV[1], s));
        assemble_variant_values(ctx, xy, vbat, s);
        HIPCHK(hipEventRecord(ctx->evV[2], s));
        HIPCHK(ctx->bc_touch.reserve((size_t)N + 16));
        magk::rhs_variants(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), ctx->v_kval.as<double>(), ctx->uknown.as<uint8_t>(), uin,
                           fin, ctx->perm.as<uint32_t>(), ctx->bc_touch.as<uint8_t>(), ctx->bc_touch_ready, N, vbat, bP, s);
        HIPCHK(hipEventRecord(ctx->evV[3], s));
        P.xyP = ctx->v_xyP.as<double2>();
        P.halo_xy = ctx->v_halo.as<double2>();
        P.var_mat = ctx->v_cmat.as<double>() + 3 * (size_t)c0;
        P.var_halo_stride = halo;
        P.var_kb_stride = kb_words;
        P.var_ovf_stride = ovf_words;
        if (eb_mode) {
            P.kblocks = ctx->v_kblocks.as<double>();
            P.kb_stride = npad;
            if (eb_mode == 2) P.ovf_rec = ctx->v_ovf.as<double>();
            magk::edge_blocks_build(P, ctx->B, nullptr, eb_mode, n, s);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->evV[4], s));
        P.bP = (const double2 *)bP;
        P.x = (double2 *)xP;
        return MAG_OK;
    };
    // scatter-back, reactions (this chunk's K) and stress (the variant's geometry and material); a variant that is redone
    // afterwards gets all three again from its own solve
    h.after_launch = [&](int32_t c0, int32_t) -> int {
        HIPCHK(hipEventRecord(ctx->evV[5], s));
        magk::post_variants(xP, ctx->perm.as<uint32_t>(), ctx->uknown.as<uint8_t>(), uin, fin, ctx->bptr.as<int32_t>(),
                            ctx->bcol.as<int32_t>(), ctx->v_kval.as<double>(), xy, ctx->conn.as<int32_t>(), N, E, vbat,
                            set.u.as<double>() + 2 * (size_t)N * c0, set.f.as<double>() + 2 * (size_t)N * c0,
                            (double *)(set.stress.as<char>() + eb * (size_t)c0), s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->evV[6], s));
        HIPCHK(hipStreamSynchronize(s));
        for (int k = 0; k < 6; ++k) ms_phase[k] += ev_ms(ctx->evV[k], ctx->evV[k + 1]);
        return MAG_OK;
    };
    h.solve_alone = [&](int32_t v, mag_stats &out, bool timed_out_before) {
        return solve_variant_alone(ctx, set, keep, v, out, timed_out_before);
    };
    // side by side: the phases' times summed over the chunks, the same in every variant (ms_element: the coordinate permutation;
    // ms_cg stays the variant's own launch, the block build is counted with ms_bc) -- one after another: each variant's cg time
    h.times = [&](mag_stats &cs) {
        cs.ms_element = ms_phase[0];
        cs.ms_assemble = ms_phase[1];
        cs.ms_bc = ms_phase[2] + ms_phase[3];
        cs.ms_post = ms_phase[5];
    };
    const int status = run_members(ctx, set, keep, h);
    // xyP, the halo copies and K may be a variant's: nothing of this run is reused by the entry points that would
    ctx->have_order = ctx->have_csr = false;
    return status;
}

} // namespace

int mag_run_variants(mag_ctx *ctx)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, "mag_run_variants");
    if (int rc = variants_refused(ctx)) return rc;
    if (!ctx->have_problem || !ctx->variants.have) return fail(ctx, MAG_ERR_STATE, "mag_run_variants before mag_set_variants");
    return run_variant_set(ctx, ctx->variants);
}

int mag_download_variant(mag_ctx *ctx, int32_t v, mag_result *r)
{
    return ctx ? download_member(ctx, ctx->variants, v, r, "mag_download_variant") : MAG_ERR_BAD_ARGS;
}

int mag_get_variant_stats(const mag_ctx *ctx, int32_t v, mag_stats *st)
{
    return ctx ? member_stats(ctx->variants, v, st) : MAG_ERR_BAD_ARGS;
}

int mag_get_variants_info(const mag_ctx *ctx, int32_t info[4]) { return ctx ? set_info(ctx->variants, info) : MAG_ERR_BAD_ARGS; }

int mag_assemble_csr_variant(mag_ctx *ctx, int32_t v, int64_t *nnz, int32_t *rowptr, int32_t *col, double *val)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, "mag_assemble_csr_variant");
    if (int rc = variants_refused(ctx)) return rc;
    if (!ctx->have_problem || !ctx->variants.have) return fail(ctx, MAG_ERR_STATE, "mag_assemble_csr_variant before mag_set_variants");
    if (v < 0 || v >= ctx->variants.count) return fail(ctx, MAG_ERR_BAD_ARGS, "variant %d out of range [0, %d)", (int)v, (int)ctx->variants.count);
    if (int rc = enter(ctx)) return rc;
    hipStream_t s = ctx->stream;
    // the shared tables and pattern of the uploaded mesh, then the variants' batched assembly for this one variant
    ctx->have_order = ctx->have_csr = false;
    if (int rc = ensure_order(ctx)) return rc;
    if (int rc = csr_symbolic(ctx)) return rc;
    const int64_t N = ctx->N, nz = 4 * ctx->nb;
    if (nnz) *nnz = nz;
    if (rowptr || col) {
        HIPCHK(ctx->rp_full.reserve(4 * (2 * (size_t)N + 1)));
        HIPCHK(ctx->col_full.reserve(4 * (size_t)nz));
        magk::csr_export(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), N, ctx->rp_full.as<int32_t>(), ctx->col_full.as<int32_t>(), s);
        HIPCHK(hipGetLastError());
        if (rowptr) HIPCHK(hipMemcpyAsync(rowptr, ctx->rp_full.p, 4 * (2 * (size_t)N + 1), hipMemcpyDeviceToHost, s));
        if (col) HIPCHK(hipMemcpyAsync(col, ctx->col_full.p, 4 * (size_t)nz, hipMemcpyDeviceToHost, s));
    }
    if (val) {
        const int64_t halo = std::max<int64_t>(ctx->halo_total, 1);
        magk::VariantBatch vbat = {};
        vbat.count = 1;
        vbat.mat = ctx->v_mat.as<double>() + 3 * (size_t)v;
        vbat.halo = halo;
        vbat.kval = nz;
        const double *xy = ctx->v_have_xy ? ctx->v_xy.as<double>() + 2 * (size_t)N * (size_t)v : ctx->xy.as<double>();
        HIPCHK(ctx->v_xyP.reserve(16 * (size_t)N));
        HIPCHK(ctx->v_halo.reserve(16 * (size_t)halo));
        HIPCHK(ctx->v_kval.reserve(8 * (size_t)nz));
        magk::variant_coords(xy, ctx->perm.as<uint32_t>(), ctx->halo_g.as<int32_t>(), N, ctx->use_lds ? ctx->halo_total : 0, vbat,
                             ctx->v_xyP.as<double>(), ctx->v_halo.as<double>(), s);
        assemble_variant_values(ctx, xy, vbat, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(val, ctx->v_kval.p, 8 * (size_t)nz, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    ctx->have_csr = false; // (no K of the uploaded problem was assembled)
    return MAG_OK;
}

// ---- energy and design sensitivities of the solved members of a set (sens.hip) ----
namespace {

const char *const kSetRun[3] = {"mag_run", "mag_run_cases", "mag_run_variants"};

// the checks mag_run_sensitivities and mag_download_sensitivity share, all before any HIP call; *count: the set's members
int sens_refused(mag_ctx *ctx, int32_t set, const char *fn, int32_t *count)
{
    if (set < MAG_SET_RUN || set > MAG_SET_VARIANTS) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: set %d is none of enum mag_set", fn, (int)set);
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "sensitivities run on one GPU: this context has a communicator of %d ranks", ctx->comm.nranks);
    // (variants were solved without a field and carry none: their passes wait until it is cleared)
    if (set == MAG_SET_VARIANTS && ctx->field_on) return field_refuses(ctx, fn);
    const bool ran = set == MAG_SET_RUN ? ctx->have_run : (set == MAG_SET_CASES ? ctx->cases.have_run : ctx->variants.have_run);
    if (!ctx->have_problem || !ran) return fail(ctx, MAG_ERR_STATE, "%s before a completed %s", fn, kSetRun[set]);
    *count = set == MAG_SET_RUN ? 1 : (set == MAG_SET_CASES ? ctx->cases.count : ctx->variants.count);
    return MAG_OK;
}

// The uploaded mesh and its ordering tables as the sensitivity kernels take them (mag_run_sensitivities, mag_run_adjoint).
// The ordering phase's tables of the uploaded mesh are there: every completed run of one rank has built them whole, and they
// hang on the connectivity and the uploaded coordinates only (a variants run leaves them as they are).  The node kernels'
// tile-local corner table is built from them once per ordering, where a tile's image fits the LDS.
int sens_mesh(mag_ctx *ctx, magk::SensMesh &mesh)
{
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N;
    const bool staged = ctx->cap <= magk::kMaxLdsNodes && env_int("MAG_TUNE_SENS_STAGE", 1) != 0;
    if (staged && !ctx->sens_tab_ready) {
        HIPCHK(ctx->sens_tab.reserve(4 * (size_t)std::max<int64_t>(ctx->ell_total, 1)));
        magk::fill_ell16(ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(), ctx->conn.as<int32_t>(), ctx->iperm.as<int32_t>(),
                         ctx->tile_deg.as<int32_t>(), ctx->tile_off.as<int64_t>(), ctx->tile_hoff.as<int32_t>(),
                         ctx->halo_g.as<int32_t>(), N, ctx->B, ctx->T, ctx->sens_tab.as<uint32_t>(), nullptr, nullptr, s);
        HIPCHK(hipGetLastError());
        ctx->sens_tab_ready = true;
    }
    mesh = {};
    mesh.N = N;
    mesh.E = ctx->E;
    mesh.conn = ctx->conn.as<int32_t>();
    mesh.u_known = ctx->uknown.as<uint8_t>();
    mesh.perm = ctx->perm.as<uint32_t>();
    mesh.inc_off = ctx->inc_off.as<int32_t>();
    mesh.inc = ctx->inc.as<uint32_t>();
    mesh.B = ctx->B;
    mesh.T = ctx->T;
    mesh.cap = ctx->cap;
    mesh.halo_g = ctx->halo_g.as<int32_t>();
    mesh.tile_hoff = ctx->tile_hoff.as<int32_t>();
    mesh.tile_deg = ctx->tile_deg.as<int32_t>();
    mesh.tile_off = ctx->tile_off.as<int64_t>();
    mesh.tab = staged ? ctx->sens_tab.as<uint32_t>() : nullptr;
    return MAG_OK;
}

// members per launch of those kernels: the scratch of one chunk (per_member bytes each) may take a quarter of the device memory
// that is free now; and what grid.y holds
int sens_chunk(mag_ctx *ctx, size_t per_member, int32_t M, int64_t &chunk)
{
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    chunk = std::max<int64_t>(1, (int64_t)(free_b / 4 / per_member));
    chunk = std::min<int64_t>(chunk, 32768);
    const int tuned = env_int("MAG_TUNE_SENS_CHUNK", 0);
    if (tuned >= 1) chunk = std::min<int64_t>(tuned, 32768);
    chunk = std::min<int64_t>(chunk, M);
    return MAG_OK;
}

// The solved members of a set as a pass reads them: where the set's run left their arrays, member after member (a stride of
// 0: every member reads the same array).
struct MemberView {
    int64_t N = 0;
    const double *xy = nullptr, *mat = nullptr, *u = nullptr, *f = nullptr, *u_in = nullptr, *f_in = nullptr;
    const double *scale = nullptr; // the element stiffness field, shared by the members (variants have none)
    int64_t xy_stride = 0, mat_stride = 0, loads_stride = 0; // doubles
    // the head of the batch of members c0 .. c0 + count - 1
    void head(magk::MemberBatch &mb, int32_t c0, int32_t count) const
    {
        mb.count = count;
        mb.mat_stride = mat_stride;
        mb.mat = mat + (size_t)mat_stride * c0;
        mb.xy_stride = xy_stride;
        mb.xy = xy + (size_t)xy_stride * c0;
        mb.u = u + 2 * (size_t)N * c0;
        mb.scale = scale;
    }
};

// The material: a variant's own (v_mat, on the device since mag_set_variants), otherwise the uploaded one for every member,
// which goes to the device here.
int member_view(mag_ctx *ctx, int32_t set, MemberView &mv)
{
    const MemberSet *ms = set == MAG_SET_CASES ? &ctx->cases : (set == MAG_SET_VARIANTS ? &ctx->variants : nullptr);
    const bool own_xy = set == MAG_SET_VARIANTS && ctx->v_have_xy, own_mat = set == MAG_SET_VARIANTS;
    const bool own_loads = set == MAG_SET_CASES || (set == MAG_SET_VARIANTS && ctx->v_have_loads);
    mv.N = ctx->N;
    mv.scale = set == MAG_SET_VARIANTS ? nullptr : field_of(ctx);
    mv.xy = own_xy ? ctx->v_xy.as<double>() : ctx->xy.as<double>();
    mv.xy_stride = own_xy ? 2 * ctx->N : 0;
    mv.u = ms ? ms->u.as<double>() : ctx->u.as<double>();
    mv.f = ms ? ms->f.as<double>() : ctx->f.as<double>();
    mv.u_in = own_loads ? ms->uin.as<double>() : ctx->uin.as<double>();
    mv.f_in = own_loads ? ms->fin.as<double>() : ctx->fin.as<double>();
    mv.loads_stride = own_loads ? 2 * ctx->N : 0;
    if (!own_mat) {
        const double mat[3] = {ctx->youngs, ctx->nu, ctx->thick};
        HIPCHK(ctx->sens_mat.reserve(sizeof mat));
        HIPCHK(hipMemcpy(ctx->sens_mat.p, mat, sizeof mat, hipMemcpyHostToDevice));
    }
    mv.mat = own_mat ? ctx->v_mat.as<double>() : ctx->sens_mat.as<double>();
    mv.mat_stride = own_mat ? 3 : 0;
    return MAG_OK;
}

struct Rows {
    DevBuf *buf;
    size_t bytes;     // per member
    const char *name; // in the message of a failed reservation
};
#define ROWS(buf, bytes) Rows{&(buf), (bytes), #buf}

int reserve_rows(mag_ctx *ctx, std::initializer_list<Rows> rows, size_t members)
{
    for (const Rows &r : rows) {
        const hipError_t e = r.buf->reserve(r.bytes * members);
        if (e != hipSuccess)
            return fail(ctx, MAG_ERR_HIP, "%s.reserve(%zu) failed: %s", r.name, r.bytes * members, hipGetErrorString(e));
    }
    return MAG_OK;
}

// The members of a pass in chunks: per_member = the scratch bytes one member needs; `results` hold all M members, `scratch`
// ONE chunk of them; launch(c0, count) fills a batch for the members from c0 and launches the pass on it.
int run_chunks(mag_ctx *ctx, DerivedSet &out, int32_t M, size_t per_member, std::initializer_list<Rows> results,
               std::initializer_list<Rows> scratch, const std::function<int(int32_t, int32_t)> &launch)
{
    int64_t chunk = 1;
    if (int rc = sens_chunk(ctx, per_member, M, chunk)) return rc;
    if (int rc = reserve_rows(ctx, results, (size_t)M)) return rc;
    HIPCHK(out.scalars.reserve(64 * (size_t)M));
    if (int rc = reserve_rows(ctx, scratch, (size_t)chunk)) return rc;
    for (int32_t c0 = 0; c0 < M; c0 += (int32_t)chunk) {
        if (int rc = launch(c0, (int32_t)std::min<int64_t>(chunk, M - c0))) return rc;
        HIPCHK(hipGetLastError());
    }
    return MAG_OK;
}

// the end of a pass: its scalars on the host, the set held
int hold_derived(mag_ctx *ctx, DerivedSet &out, int32_t M)
{
    hipStream_t s = ctx->stream;
    out.scalars_h.assign(8 * (size_t)M, 0.0);
    HIPCHK(hipMemcpyAsync(out.scalars_h.data(), out.scalars.p, 64 * (size_t)M, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    out.count = M;
    out.have = true;
    return MAG_OK;
}

// The checks of a pass's mag_download_* (fn; `sets`: the pass's results, which the entry point run_fn leaves; what: the caller's
// struct in messages), all before any HIP call; *have: the results of the set
int download_refused(mag_ctx *ctx, Pass pass, int32_t set, int32_t index, const void *o, const char *what,
                     const char *fn, const char *run_fn, const DerivedSet **have)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "null %s", what);
    if (index < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "member %d out of range", (int)index);
    int32_t M = 0;
    if (int rc = sens_refused(ctx, set, fn, &M)) return rc;
    *have = &ctx->derived[pass][set];
    if (!(*have)->have) return fail(ctx, MAG_ERR_STATE, "%s before %s of this set", fn, run_fn);
    if (index >= (*have)->count) return fail(ctx, MAG_ERR_BAD_ARGS, "member %d out of range [0, %d)", (int)index, (int)(*have)->count);
    return MAG_OK;
}

struct Download {
    void *dst; // the caller's, or null: not wanted
    const DevBuf &src;
    size_t bytes; // per member
};

// ... and past them: the rows of member `index` to the caller's memory, the eight scalars
int download_rows(mag_ctx *ctx, const DerivedSet &have, int32_t index, int32_t memory, std::initializer_list<Download> rows, double *scalars)
{
    if (int rc = enter(ctx)) return rc;
    const hipMemcpyKind kind = memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipStream_t s = ctx->stream;
    const size_t i = (size_t)index;
    for (const Download &r : rows)
        if (r.dst) HIPCHK(hipMemcpyAsync(r.dst, r.src.as<char>() + r.bytes * i, r.bytes, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < 8; ++k) scalars[k] = have.scalars_h[8 * i + k];
    return MAG_OK;
}

} // namespace

int mag_run_sensitivities(mag_ctx *ctx, int32_t set)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    int32_t M = 0;
    if (int rc = sens_refused(ctx, set, "mag_run_sensitivities", &M)) return rc;
    if (int rc = enter(ctx)) return rc;
    const int64_t N = ctx->N, E = ctx->E;
    const size_t vb = 16 * (size_t)N, eb = 8 * (size_t)E, pb = 8 * 4 * (size_t)magk::kSensBlocks;
    DerivedSet &out = ctx->derived[PASS_SENS][set];
    out.have = false;
    magk::SensMesh mesh;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    MemberView mv;
    if (int rc = member_view(ctx, set, mv)) return rc;
    const auto launch = [&](int32_t c0, int32_t count) {
        magk::SensBatch sb = {};
        mv.head(sb, c0, count);
        sb.f_out = mv.f + 2 * (size_t)N * c0;
        sb.loads_stride = mv.loads_stride;
        sb.u_in = mv.u_in + (size_t)mv.loads_stride * c0;
        sb.f_in = mv.f_in + (size_t)mv.loads_stride * c0;
        sb.energy = out.energy.as<double>() + (size_t)E * c0;
        sb.dxy = out.dxy.as<double>() + 2 * (size_t)N * c0;
        sb.scalars = out.scalars.as<double>() + 8 * (size_t)c0;
        sb.nuterm = ctx->sens_nuterm.as<double>();
        sb.partials = ctx->sens_part.as<double>();
        magk::sensitivities(mesh, sb, ctx->stream);
        return (int)MAG_OK;
    };
    // (the scratch of one member: a nu term per element, the partial sums)
    if (int rc = run_chunks(ctx, out, M, eb + pb, {ROWS(out.energy, eb), ROWS(out.dxy, vb)}, {ROWS(ctx->sens_nuterm, eb), ROWS(ctx->sens_part, pb)}, launch))
        return rc;
    return hold_derived(ctx, out, M);
}

int mag_download_sensitivity(mag_ctx *ctx, int32_t set, int32_t index, mag_sensitivity *o)
{
    const DerivedSet *have = nullptr;
    if (ctx && o)
        if (int rc = memory_refused(ctx, o->memory, "mag_download_sensitivity")) return rc;
    if (int rc = download_refused(ctx, PASS_SENS, set, index, o, "sensitivity", "mag_download_sensitivity", "mag_run_sensitivities", &have))
        return rc;
    const size_t eb = 8 * (size_t)ctx->E, vb = 16 * (size_t)ctx->N;
    return download_rows(ctx, *have, index, o->memory, {{o->energy_out, have->energy, eb}, {o->dxy_out, have->dxy, vb}}, o->scalars);
}

// ---- adjoint sensitivities of the solved members of a set: the adjoint systems through the member-set driver, then the
// bilinear pass (adjoint.hip) ----
namespace {

// What a set's run drops of the single-case path (begin_run) and overwrites in its buffers: kept aside around the run of an
// adjoint set, which must leave all of it as it was.
struct KeptRun {
    mag_ctx *ctx;
    const size_t vb, eb;
    const mag_stats stats;
    const bool have_run;
    bool have_derived[PASS_COUNT]; // (of the single case)
    const int32_t history_len;
    bool armed = false;
    explicit KeptRun(mag_ctx *c)
        : ctx(c), vb(16 * (size_t)c->N), eb(8 * (size_t)c->E), stats(c->stats), have_run(c->have_run), history_len(c->opt.history_len)
    {
        for (int k = 0; k < PASS_COUNT; ++k) have_derived[k] = ctx->derived[k][MAG_SET_RUN].have;
    }
    int keep() // (u, f, stress: the CSR operator's phase expands into the context's u, a lent problem runs through all three)
    {
        ctx->opt.history_len = 0; // the recorded costs stay those of the run that recorded them
        if (!have_run) return MAG_OK;
        hipStream_t s = ctx->stream;
        HIPCHK(ctx->adj_keep.reserve(2 * vb + eb));
        HIPCHK(hipMemcpyAsync(ctx->adj_keep.p, ctx->u.p, vb, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->adj_keep.as<char>() + vb, ctx->f.p, vb, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->adj_keep.as<char>() + 2 * vb, ctx->stress.p, eb, hipMemcpyDeviceToDevice, s));
        armed = true;
        return MAG_OK;
    }
    ~KeptRun()
    {
        ctx->opt.history_len = history_len;
        ctx->stats = stats;
        ctx->have_run = have_run;
        for (int k = 0; k < PASS_COUNT; ++k) ctx->derived[k][MAG_SET_RUN].have = have_derived[k];
        if (!armed) return;
        hipStream_t s = ctx->stream;
        (void)hipMemcpyAsync(ctx->u.p, ctx->adj_keep.p, vb, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(ctx->f.p, ctx->adj_keep.as<char>() + vb, vb, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(ctx->stress.p, ctx->adj_keep.as<char>() + 2 * vb, eb, hipMemcpyDeviceToDevice, s);
        (void)hipStreamSynchronize(s);
    }
};

// mag_run_adjoint past its checks: dJ_du [M][2N] on the host or -- mag_run_objective's -- already on the device
int run_adjoint(mag_ctx *ctx, int32_t set, int32_t M, const double *dJ_du, int32_t memory)
{
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N, E = ctx->E;
    const size_t vb = 16 * (size_t)N;
    DerivedSet &out = ctx->derived[PASS_ADJOINT][set];
    MemberSet &adj = ctx->adj[set];
    out.have = false;
    adj.have = adj.have_run = false;
    // the adjoint systems: load sets (0, dJ/du) on the set's own K
    HIPCHK(adj.uin.reserve(vb * M));
    HIPCHK(adj.fin.reserve(vb * M));
    HIPCHK(hipMemsetAsync(adj.uin.p, 0, vb * M, s));
    HIPCHK(hipMemcpyAsync(adj.fin.p, dJ_du, vb * M, memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    adj.count = M;
    adj.have = true;
    int status = MAG_OK;
    {
        KeptRun kept(ctx);
        if (int rc = kept.keep()) return rc;
        status = set == MAG_SET_VARIANTS ? run_variant_set(ctx, adj) : run_case_set(ctx, adj);
    }
    if (status != MAG_OK && status != MAG_ERR_NOT_CONVERGED) return status;
    const std::string run_message = ctx->err;

    // ---- the bilinear pass over (u of the set, lambda = u of its adjoint set), chunked as mag_run_sensitivities is
    const size_t eb = 8 * (size_t)E, pb = 8 * 2 * (size_t)magk::kSensBlocks;
    magk::SensMesh mesh;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    MemberView mv;
    if (int rc = member_view(ctx, set, mv)) return rc;
    const auto launch = [&](int32_t c0, int32_t count) {
        magk::AdjointBatch ab = {};
        mv.head(ab, c0, count);
        ab.lam = adj.u.as<double>() + 2 * (size_t)N * c0;
        ab.g = adj.fin.as<double>() + 2 * (size_t)N * c0;
        ab.f_adj = adj.f.as<double>() + 2 * (size_t)N * c0;
        ab.dloads = out.dloads.as<double>() + 2 * (size_t)N * c0;
        ab.delem = out.delem.as<double>() + (size_t)E * c0;
        ab.dxy = out.dxy.as<double>() + 2 * (size_t)N * c0;
        ab.scalars = out.scalars.as<double>() + 8 * (size_t)c0;
        ab.nuterm = ctx->sens_nuterm.as<double>();
        ab.partials = ctx->sens_part.as<double>();
        HIPCHK(magk::adjoint_bilinear(mesh, ab, s));
        return (int)MAG_OK;
    };
    if (int rc = run_chunks(ctx, out, M, eb + pb, {ROWS(out.dloads, vb), ROWS(out.delem, eb), ROWS(out.dxy, vb)},
                            {ROWS(ctx->sens_nuterm, eb), ROWS(ctx->sens_part, pb)}, launch))
        return rc;
    if (int rc = hold_derived(ctx, out, M)) return rc;
    if (status != MAG_OK) ctx->err = run_message;
    return status;
}

} // namespace

int mag_run_adjoint(mag_ctx *ctx, int32_t set, const double *dJ_du, int32_t memory)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    int32_t M = 0;
    if (set >= MAG_SET_RUN && set <= MAG_SET_VARIANTS && !dJ_du) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_adjoint: null dJ_du");
    if (dJ_du)
        if (int rc = memory_refused(ctx, memory, "mag_run_adjoint")) return rc;
    if (int rc = sens_refused(ctx, set, "mag_run_adjoint", &M)) return rc;
    if (int rc = enter(ctx)) return rc;
    return run_adjoint(ctx, set, M, dJ_du, memory);
}

int mag_download_adjoint(mag_ctx *ctx, int32_t set, int32_t index, mag_adjoint *o)
{
    const DerivedSet *have = nullptr;
    if (ctx && o)
        if (int rc = memory_refused(ctx, o->memory, "mag_download_adjoint")) return rc;
    if (int rc = download_refused(ctx, PASS_ADJOINT, set, index, o, "adjoint", "mag_download_adjoint", "mag_run_adjoint", &have)) return rc;
    const size_t eb = 8 * (size_t)ctx->E, vb = 16 * (size_t)ctx->N;
    return download_rows(ctx, *have, index, o->memory,
                         {{o->lambda_out, ctx->adj[set].u, vb}, {o->dloads_out, have->dloads, vb}, {o->delem_out, have->delem, eb},
                          {o->dxy_out, have->dxy, vb}},
                         o->scalars);
}

int mag_get_adjoint_stats(const mag_ctx *ctx, int32_t set, int32_t index, mag_stats *st)
{
    if (!ctx || !st || index < 0 || set < MAG_SET_RUN || set > MAG_SET_VARIANTS || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->derived[PASS_ADJOINT][set].have) return MAG_ERR_STATE;
    return member_stats(ctx->adj[set], index, st);
}

int mag_get_adjoint_info(const mag_ctx *ctx, int32_t set, int32_t info[4])
{
    if (!ctx || !info || set < MAG_SET_RUN || set > MAG_SET_VARIANTS || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->derived[PASS_ADJOINT][set].have) return MAG_ERR_STATE;
    return set_info(ctx->adj[set], info);
}

// ---- objectives of the solved members of a set on the device (objective.hip): J, dJ/du, the explicit partials; with_adjoint,
// dJ/du goes on to the adjoint pass where it lies and the totals are formed ----
int mag_run_objective(mag_ctx *ctx, int32_t set, const mag_objective *obj, int32_t with_adjoint)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (set < MAG_SET_RUN || set > MAG_SET_VARIANTS)
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_objective: set %d is none of enum mag_set", (int)set);
    if (!obj) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_objective: null objective");
    if (obj->kind != MAG_OBJ_DISP_LSQ && obj->kind != MAG_OBJ_STRESS_PNORM)
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_objective: kind %d is none of enum mag_objective_kind", (int)obj->kind);
    const bool lsq = obj->kind == MAG_OBJ_DISP_LSQ;
    if (obj->weights || (lsq && obj->target)) // (the rows that would be read)
        if (int rc = memory_refused(ctx, obj->memory, "mag_run_objective")) return rc;
    if (lsq && !obj->weights) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_objective: MAG_OBJ_DISP_LSQ needs weights");
    if (!lsq && !(std::isfinite(obj->p) && obj->p >= 1.0))
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_objective: p = %g is not a finite exponent >= 1", obj->p);
    if (!lsq && !(std::isfinite(obj->scale) && obj->scale > 0.0))
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_objective: scale = %g is not a finite stress > 0", obj->scale);
    int32_t M = 0;
    if (int rc = sens_refused(ctx, set, "mag_run_objective", &M)) return rc;
    if (int rc = enter(ctx)) return rc;
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N, E = ctx->E;
    const size_t vb = 16 * (size_t)N;
    DerivedSet &out = ctx->derived[PASS_OBJECTIVE][set];
    out.have = out.totals = false;
    magk::SensMesh mesh;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    MemberView mv;
    if (int rc = member_view(ctx, set, mv)) return rc;
    // the caller's rows: one for all members or one per member, on the device as they are
    const int64_t row = lsq ? 2 * N : E, stride = obj->per_member ? row : 0;
    const size_t rows_b = 8 * (size_t)row * (obj->per_member ? (size_t)M : 1);
    const double *w = obj->weights, *target = lsq ? obj->target : nullptr;
    if (obj->memory != MAG_MEM_DEVICE) {
        if (w) {
            HIPCHK(ctx->obj_w.reserve(rows_b));
            HIPCHK(hipMemcpyAsync(ctx->obj_w.p, w, rows_b, hipMemcpyHostToDevice, s));
            w = ctx->obj_w.as<double>();
        }
        if (target) {
            HIPCHK(ctx->obj_target.reserve(rows_b));
            HIPCHK(hipMemcpyAsync(ctx->obj_target.p, target, rows_b, hipMemcpyHostToDevice, s));
            target = ctx->obj_target.as<double>();
        }
    }
    const auto launch = [&](int32_t c0, int32_t count) {
        magk::ObjectiveBatch ob = {};
        mv.head(ob, c0, count);
        ob.kind = obj->kind;
        ob.w_stride = stride;
        ob.w = w ? w + (size_t)stride * c0 : nullptr;
        ob.target_stride = stride;
        ob.target = target ? target + (size_t)stride * c0 : nullptr;
        ob.p = obj->p;
        ob.scale = obj->scale;
        ob.g = out.g.as<double>() + 2 * (size_t)N * c0;
        ob.pxy = out.pxy.as<double>() + 2 * (size_t)N * c0;
        ob.scalars = out.scalars.as<double>() + 8 * (size_t)c0;
        ob.terms = ctx->obj_terms.as<double>();
        ob.nuterm = ctx->sens_nuterm.as<double>();
        ob.helem = ctx->obj_helem.as<double>();
        ob.partials = ctx->sens_part.as<double>();
        ob.factor = ctx->obj_factor.as<double>();
        magk::objective(mesh, ob, s);
        return (int)MAG_OK;
    };
    // (the scratch of one member: summands, nu terms and factors per element, the partial sums, the member's factor)
    const size_t eb = 8 * (size_t)E, tb = 8 * (size_t)row, pb = 8 * 2 * (size_t)magk::kSensBlocks;
    if (int rc = run_chunks(ctx, out, M, tb + 2 * eb + pb + 8, {ROWS(out.g, vb), ROWS(out.pxy, vb)},
                            {ROWS(ctx->obj_terms, tb), ROWS(ctx->sens_nuterm, eb), ROWS(ctx->obj_helem, eb), ROWS(ctx->sens_part, pb), ROWS(ctx->obj_factor, 8)},
                            launch))
        return rc;
    HIPCHK(hipStreamSynchronize(s)); // (the caller's rows are read, the results stand)
    out.count = M;
    out.have = true;
    int status = MAG_OK;
    std::string run_message;
    if (with_adjoint) {
        status = run_adjoint(ctx, set, M, out.g.as<double>(), MAG_MEM_DEVICE);
        if (status != MAG_OK && status != MAG_ERR_NOT_CONVERGED) return status;
        run_message = ctx->err;
        const DerivedSet &adj = ctx->derived[PASS_ADJOINT][set];
        HIPCHK(out.dxy.reserve(vb * M));
        magk::objective_totals(N, M, out.pxy.as<double>(), adj.dxy.as<double>(), adj.scalars.as<double>(), out.dxy.as<double>(),
                               out.scalars.as<double>(), s);
        HIPCHK(hipGetLastError());
    }
    if (int rc = hold_derived(ctx, out, M)) return rc;
    out.totals = with_adjoint != 0;
    if (status != MAG_OK) ctx->err = run_message;
    return status;
}

int mag_download_objective(mag_ctx *ctx, int32_t set, int32_t index, mag_objective_result *o)
{
    const DerivedSet *have = nullptr;
    if (ctx && o)
        if (int rc = memory_refused(ctx, o->memory, "mag_download_objective")) return rc;
    if (int rc = download_refused(ctx, PASS_OBJECTIVE, set, index, o, "objective result", "mag_download_objective", "mag_run_objective", &have))
        return rc;
    if (o->dxy_out && !have->totals)
        return fail(ctx, MAG_ERR_STATE, "mag_download_objective: dxy_out needs mag_run_objective with with_adjoint != 0");
    const size_t vb = 16 * (size_t)ctx->N;
    return download_rows(ctx, *have, index, o->memory, {{o->g_out, have->g, vb}, {o->pxy_out, have->pxy, vb}, {o->dxy_out, have->dxy, vb}},
                         o->scalars);
}

// ---- stress recovery of the solved members of a set (recover.hip): the fourth pass, chunked as mag_run_sensitivities is ----
int mag_run_stress(mag_ctx *ctx, int32_t set)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, "mag_run_stress");
    int32_t M = 0;
    if (int rc = sens_refused(ctx, set, "mag_run_stress", &M)) return rc;
    if (int rc = enter(ctx)) return rc;
    const int64_t N = ctx->N, E = ctx->E;
    const size_t nb = 32 * (size_t)N, rb = 32 * (size_t)E, eb = 8 * (size_t)E, pb = 8 * 4 * (size_t)magk::kSensBlocks;
    DerivedSet &out = ctx->derived[PASS_STRESS][set];
    out.have = false;
    magk::SensMesh mesh;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    MemberView mv;
    if (int rc = member_view(ctx, set, mv)) return rc;
    const auto launch = [&](int32_t c0, int32_t count) {
        magk::StressBatch sb = {};
        mv.head(sb, c0, count);
        sb.elem = out.selem.as<double>() + 4 * (size_t)E * c0;
        sb.node = out.snode.as<double>() + 4 * (size_t)N * c0;
        sb.eta2 = out.seta2.as<double>() + (size_t)E * c0;
        sb.scalars = out.scalars.as<double>() + 8 * (size_t)c0;
        sb.uterm = ctx->sens_nuterm.as<double>();
        sb.partials = ctx->sens_part.as<double>();
        magk::stress_recovery(mesh, sb, ctx->stream);
        return (int)MAG_OK;
    };
    // (the scratch of one member: an energy term per element, the partial sums and maxima -- the sensitivities' buffers)
    if (int rc = run_chunks(ctx, out, M, eb + pb, {ROWS(out.selem, rb), ROWS(out.snode, nb), ROWS(out.seta2, eb)},
                            {ROWS(ctx->sens_nuterm, eb), ROWS(ctx->sens_part, pb)}, launch))
        return rc;
    return hold_derived(ctx, out, M);
}

int mag_download_stress(mag_ctx *ctx, int32_t set, int32_t index, mag_stress_field *o)
{
    const DerivedSet *have = nullptr;
    if (ctx && o)
        if (int rc = memory_refused(ctx, o->memory, "mag_download_stress")) return rc;
    if (int rc = download_refused(ctx, PASS_STRESS, set, index, o, "stress field", "mag_download_stress", "mag_run_stress", &have)) return rc;
    const size_t rb = 32 * (size_t)ctx->E, nb = 32 * (size_t)ctx->N, eb = 8 * (size_t)ctx->E;
    return download_rows(ctx, *have, index, o->memory, {{o->elem_out, have->selem, rb}, {o->node_out, have->snode, nb}, {o->eta2_out, have->seta2, eb}},
                         o->scalars);
}

// ---- the subspace iteration of modal analysis and of linearised buckling (modal.hip, buckling.hip, modal_host.h): the pairs of
// K_FF phi = lambda S_FF phi at the lower end, S the pass's second operator (the mass M; minus the geometric stiffness K_G), the
// inner solves through the member-set driver as one more set, the Rayleigh-Ritz step on the host.  One driver, two callers ----
namespace {

// The inner solves of the iteration run under MAG_STOP_REL with cg_tol, silently: the context's stop rule, tolerance and
// verbosity (read at every solve) are swapped here and come back on every exit path; the history is KeptRun's.
struct ModalStopRule {
    mag_ctx *ctx;
    const int32_t stop_mode, verbose;
    const double tol;
    ModalStopRule(mag_ctx *c, double cg_tol) : ctx(c), stop_mode(c->opt.stop_mode), verbose(c->opt.verbose), tol(c->opt.tol)
    {
        ctx->opt.stop_mode = MAG_STOP_REL;
        ctx->opt.tol = cg_tol;
        ctx->opt.verbose = 0;
    }
    ~ModalStopRule()
    {
        ctx->opt.stop_mode = stop_mode;
        ctx->opt.tol = tol;
        ctx->opt.verbose = verbose;
    }
};

// the checks of the mass operator's arguments (mag_run_modal, mag_apply_mass), before any HIP call
int mass_refused(mag_ctx *ctx, const char *fn, double density)
{
    if (!(density > 0.0) || !std::isfinite(density)) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: density %g is not positive and finite", fn, density);
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "modal analysis runs on one GPU: this context has a communicator of %d ranks", ctx->comm.nranks);
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "%s before mag_upload", fn);
    return MAG_OK;
}

// `count` vectors x on the uploaded mesh as the mass pass takes them (one mesh, one material, many vectors)
int mass_batch(mag_ctx *ctx, double density, int32_t lumped, int32_t masked, int32_t count, const double *x, double *y, magk::MassBatch &mb)
{
    MemberView mv;
    if (int rc = member_view(ctx, MAG_SET_RUN, mv)) return rc; // (the uploaded material, on the device)
    mb = {};
    mb.count = count;
    mb.mat = mv.mat;
    mb.mat_stride = 0;
    mb.xy = ctx->xy.as<double>();
    mb.xy_stride = 0;
    mb.u = x;
    mb.y = y;
    mb.density = density;
    mb.lumped = lumped ? 1 : 0;
    mb.masked = masked ? 1 : 0;
    return MAG_OK;
}

// ... and as the geometric stiffness pass takes them, under the prestress u0 (2N, on the device)
int geometric_batch(mag_ctx *ctx, const double *u0, double sign, int32_t masked, int32_t count, const double *x, double *y, magk::GeomBatch &gb)
{
    MemberView mv;
    if (int rc = member_view(ctx, MAG_SET_RUN, mv)) return rc; // (the uploaded material, on the device)
    gb = {};
    gb.count = count;
    gb.mat = mv.mat;
    gb.mat_stride = 0;
    gb.xy = ctx->xy.as<double>();
    gb.xy_stride = 0;
    gb.u = x;
    gb.u0 = u0;
    gb.y = y;
    gb.sign = sign;
    gb.masked = masked ? 1 : 0;
    return MAG_OK;
}

// What a pass hands the driver: its name for messages, its state, the sizes and tolerances (defaults filled in) and
//   second(mesh, count, x, y)        enqueues y = S x for `count` vectors, rows of prescribed DOFs zero (mesh: the tables as they
//                                    are now -- a run of the set redoes the ordering),
//   ritz(step, A, B, values, Q)      the Rayleigh-Ritz step on A = Z^T K Z and B = Z^T S Z (q x q, symmetrised): the q values by
//                                    which convergence is judged and the residual formed, in the pass's order, and Q (column k =
//                                    Ritz vector k); MAG_OK, or the status with the message set,
//   start(Y, norms)                  (may be empty) judges the start Y = S X in front of the first inner solve; norms: device
//                                    scratch of 2 q doubles,
//   first_gram(A)                    (may be empty) judges the first step's A in front of its Ritz step,
//   k_normalise                      the pass normalises its shapes by K (buckling: through A = Z^T Y, which stands for Z^T K Z only
//                                    as far as the inner solves reach K Z = Y): the shapes are normalised once more at the end, by
//                                    one product K X (k_normalise_shapes).
struct SubspaceProblem {
    const char *fn;
    SubspacePass &pass;
    int32_t p, q, max_outer;
    double tol, cg_tol;
    std::function<int(const magk::SensMesh &, int32_t, const double *, double *)> second;
    std::function<int(int32_t, const double *, const double *, double *, double *)> ritz;
    std::function<int(const double *, double *)> start;
    std::function<int(const double *)> first_gram;
    bool k_normalise = false;
};

// the status of a Ritz function of modal_host.h under the pass's name (hint: what the pass adds on dependent vectors)
int ritz_status(mag_ctx *ctx, const char *fn, int32_t step, int eig, int pivot, double least, const char *hint)
{
    if (eig == magh::EIG_DEPENDENT)
        return fail(ctx, MAG_ERR_NOT_CONVERGED,
                    "%s: outer step %d: the vectors of the subspace are linearly dependent (pivot %d of the Gram matrices: %.3g against a "
                    "unit diagonal, refused at or below %.3g)%s",
                    fn, (int)step + 1, pivot, least, magh::kEigPivotTol, hint);
    if (eig != magh::EIG_OK) return fail(ctx, MAG_ERR_NOT_CONVERGED, "%s: outer step %d: the Rayleigh-Ritz step did not converge", fn, (int)step + 1);
    return MAG_OK;
}

// X^T K X = I for the p shapes X of a pass that normalises by K, exactly: G = X^T (K_FF X) by one matrix-free product per shape
// (mag_apply_operator's path, in the CG's scratch vectors) and the Gram kernel, G = L L^T on the host, X <- X L^-T and Y <- Y L^-T
// by the rotation kernel.  Through A = Z^T Y alone the shapes are K-orthonormal as far as the inner solves reach K Z = Y: where
// Y = -K_G X is rough and Z smooth, |Z| |Y| / Z^T Y is large and a CG residual of 1e-12 |Y| left 1.7e-10 on a 16:1 column.
// The correction is of that size: the factors and the residual vectors stay.
int k_normalise_shapes(mag_ctx *ctx, const char *fn, SubspacePass &ps, int32_t p, double *Y, double *Y2, double *d_qs, double *d_gram)
{
    constexpr int MQ = magk::kModalMaxQ;
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N;
    const size_t vb = 16 * (size_t)N;
    double *X = ps.x.as<double>(), *KX = ps.w.as<double>();
    if (int rc = ensure_full_order(ctx)) return rc;
    if (int rc = reserve_cg(ctx)) return rc;
    for (int32_t k = 0; k < p; ++k) {
        magk::to_hilbert(X + 2 * N * k, ctx->iperm.as<int32_t>(), ctx->uknown.as<uint8_t>(), 1, N, ctx->tmpP.as<double>(), s);
        if (int rc = apply_plain(ctx, ctx->tmpP.as<double>(), ctx->q.as<double>(), 1)) return rc;
        magk::from_hilbert(ctx->q.as<double>(), ctx->iperm.as<int32_t>(), N, KX + 2 * N * k, s);
    }
    std::vector<double> G(2 * (size_t)p * p), L((size_t)p * p, 0.0), h_qs(MQ * MQ + MQ, 0.0);
    magk::gram(X, KX, KX, N, p, ps.part.as<double>(), d_gram, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(G.data(), d_gram, 8 * G.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int32_t j = 0; j < p; ++j) { // G = L L^T on the mean of both triangles
        double d = G[(size_t)j * p + j];
        for (int32_t k = 0; k < j; ++k) d -= L[(size_t)j * p + k] * L[(size_t)j * p + k];
        if (!(d > 0.0) || !std::isfinite(d))
            return fail(ctx, MAG_ERR_NOT_CONVERGED, "%s: the shapes are not independent in K's inner product (pivot %d: %.3g)", fn, (int)j, d);
        L[(size_t)j * p + j] = std::sqrt(d);
        for (int32_t i = j + 1; i < p; ++i) {
            double t = 0.5 * (G[(size_t)i * p + j] + G[(size_t)j * p + i]);
            for (int32_t k = 0; k < j; ++k) t -= L[(size_t)i * p + k] * L[(size_t)j * p + k];
            L[(size_t)i * p + j] = t / L[(size_t)j * p + j];
        }
    }
    for (int32_t k = 0; k < p; ++k) { // column k of L^-T: L^T c = e_k, from the last row up (upper triangular: zero below k)
        double c[MQ] = {};
        for (int32_t i = k; i >= 0; --i) {
            double t = i == k ? 1.0 : 0.0;
            for (int32_t m = i + 1; m <= k; ++m) t -= L[(size_t)m * p + i] * c[m];
            c[i] = t / L[(size_t)i * p + i];
        }
        for (int32_t i = 0; i <= k; ++i) h_qs[(size_t)i * MQ + k] = c[i];
    }
    HIPCHK(hipMemcpyAsync(d_qs, h_qs.data(), 8 * h_qs.size(), hipMemcpyHostToDevice, s));
    magk::rotate(X, Y, Y, d_qs, N, p, p, KX, Y2, nullptr, s); // (K X is done with: the new shapes go there first)
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(X, KX, vb * p, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(Y, Y2, vb * p, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s)); // (h_qs is done with)
    return MAG_OK;
}

// The iteration, past the pass's argument checks and inside the context: the ordering, the orientation check, the buffers, the
// start vectors, the outer steps, the residuals and signs; leaves pass.have, pass.info[0..6], pass.lambda (the first p values)
// and pass.residual.
int subspace_iteration(mag_ctx *ctx, const SubspaceProblem &sp)
{
    const char *fn = sp.fn;
    SubspacePass &ps = sp.pass;
    const int32_t p = sp.p, q = sp.q, max_outer = sp.max_outer;
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N;
    const size_t vb = 16 * (size_t)N;
    constexpr int MQ = magk::kModalMaxQ;
    ps.have = false;
    MemberSet &set = ps.set;
    set.have = set.have_run = false;

    if (int rc = ensure_full_order(ctx)) return rc; // (validates conn, counts the free DOFs, leaves the bounding box)
    if (q > ctx->nf) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: subspace = %d exceeds the %lld free DOFs", fn, (int)q, (long long)ctx->nf);
    HIPCHK(ps.bad.reserve(8));
    unsigned long long bad = ~0ull;
    magk::orientation(ctx->xy.as<double>(), ctx->conn.as<int32_t>(), N, ctx->E, ps.bad.as<unsigned long long>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&bad, ps.bad.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad != ~0ull)
        return fail(ctx, MAG_ERR_BAD_ARGS,
                    "%s: element %lld has a signed area <= 0 (the stiffness carries the signed area: modal analysis needs "
                    "counter-clockwise elements)",
                    fn, (long long)bad);

    // Q [MQ][MQ], lambda [MQ], then A and B [q][q] each, then the norms [q][2]
    const size_t small_doubles = MQ * MQ + MQ + 2 * (size_t)MQ * MQ + 2 * MQ;
    HIPCHK(set.uin.reserve(vb * q));
    HIPCHK(set.fin.reserve(vb * q));
    HIPCHK(ps.x.reserve(vb * q));
    HIPCHK(ps.w.reserve(vb * q));
    HIPCHK(ps.y2.reserve(vb * q));
    HIPCHK(ps.r.reserve(vb * p));
    HIPCHK(ps.part.reserve(8 * 2 * magk::kModalGramCols * (size_t)magk::kSensBlocks * (size_t)magk::gram_rows(q)));
    HIPCHK(ps.small.reserve(8 * small_doubles));
    double *d_qs = ps.small.as<double>(), *d_gram = d_qs + MQ * MQ + MQ, *d_norms = d_gram + 2 * MQ * MQ;
    double *X = ps.x.as<double>(), *Y = set.fin.as<double>(), *W = ps.w.as<double>(), *Y2 = ps.y2.as<double>();

    // ---- 1. the start vectors and Y = S X
    magk::SensMesh mesh;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    HIPCHK(hipMemsetAsync(set.uin.p, 0, vb * q, s));
    magk::start_vectors(ctx->xy.as<double>(), ctx->uknown.as<uint8_t>(), N, q, X, s);
    if (int rc = sp.second(mesh, q, X, Y)) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (sp.start)
        if (int rc = sp.start(Y, d_norms)) return rc;
    set.count = q;
    set.have = true;

    // ---- 2. the outer steps
    int32_t *info = ps.info;
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[0] = p;
    info[1] = q;
    std::vector<double> lambda((size_t)q, 0.0), prev, h_gram(2 * (size_t)q * q), A((size_t)q * q), B((size_t)q * q), Qm((size_t)q * q), h_qs(MQ * MQ + MQ);
    bool converged = false;
    for (int32_t step = 0; step < max_outer; ++step) {
        int status = MAG_OK;
        {
            KeptRun kept(ctx);
            if (int rc = kept.keep()) return rc;
            ModalStopRule rule(ctx, sp.cg_tol);
            status = run_case_set(ctx, set);
        }
        info[2] = step + 1;
        info[4] = set.info[1];
        info[5] += set.info[2];
        info[6] += set.info[3];
        if (status != MAG_OK) { // (the inner solve's own status and words, under this entry point's name)
            const std::string why = ctx->err;
            return fail(ctx, status, "%s: outer step %d: %s", fn, (int)step + 1, why.c_str());
        }
        for (int32_t j = 0; j < q; ++j)
            if (!set.stats[(size_t)j].converged)
                return fail(ctx, MAG_ERR_NOT_CONVERGED,
                            "%s: outer step %d, vector %d: the inner solve stopped at the iteration cap after %lld iterations "
                            "(a part without enough supports has a singular K_FF)",
                            fn, (int)step + 1, (int)j, (long long)set.stats[(size_t)j].iterations);
        const double *Z = set.u.as<double>();
        if (int rc = sens_mesh(ctx, mesh)) return rc; // (the run has redone the ordering: the tile-local table with it)
        if (int rc = sp.second(mesh, q, Z, W)) return rc;
        magk::gram(Z, Y, W, N, q, ps.part.as<double>(), d_gram, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_gram.data(), d_gram, 8 * h_gram.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int32_t i = 0; i < q; ++i)
            for (int32_t j = 0; j < q; ++j) {
                A[(size_t)i * q + j] = 0.5 * (h_gram[(size_t)i * q + j] + h_gram[(size_t)j * q + i]);
                B[(size_t)i * q + j] = 0.5 * (h_gram[(size_t)q * q + (size_t)i * q + j] + h_gram[(size_t)q * q + (size_t)j * q + i]);
            }
        if (step == 0 && sp.first_gram)
            if (int rc = sp.first_gram(A.data())) return rc;
        if (int rc = sp.ritz(step, A.data(), B.data(), lambda.data(), Qm.data())) return rc;
        if (!prev.empty()) {
            double change = 0.0;
            for (int32_t k = 0; k < p; ++k) change = std::max(change, std::fabs(lambda[(size_t)k] - prev[(size_t)k]) / std::fabs(lambda[(size_t)k]));
            converged = change <= sp.tol; // (a NaN is no convergence)
        }
        prev = lambda;
        const bool last = converged || step + 1 == max_outer;
        std::fill(h_qs.begin(), h_qs.end(), 0.0);
        for (int32_t i = 0; i < q; ++i)
            for (int32_t j = 0; j < q; ++j) h_qs[(size_t)i * MQ + j] = Qm[(size_t)i * q + j];
        for (int32_t k = 0; k < q; ++k) h_qs[(size_t)MQ * MQ + k] = lambda[(size_t)k];
        HIPCHK(hipMemcpyAsync(d_qs, h_qs.data(), 8 * h_qs.size(), hipMemcpyHostToDevice, s));
        magk::rotate(Z, W, Y, d_qs, N, q, p, X, Y2, last ? ps.r.as<double>() : nullptr, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(Y, Y2, vb * q, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s)); // (h_qs is done with)
        if (last) break;
    }

    // ---- 3. the residuals from the pass's own quantities, the shapes' signs
    if (sp.k_normalise)
        if (int rc = k_normalise_shapes(ctx, fn, ps, p, Y, Y2, d_qs, d_gram)) return rc;
    std::vector<double> norms(2 * (size_t)p);
    magk::residual_norms(ps.r.as<double>(), Y, N, p, ps.part.as<double>(), d_norms, s);
    magk::fix_signs(X, N, p, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(norms.data(), d_norms, 8 * norms.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ps.lambda.assign(lambda.begin(), lambda.begin() + p);
    ps.residual.assign((size_t)p, 0.0);
    for (int32_t k = 0; k < p; ++k) {
        const double den = std::fabs(lambda[(size_t)k]) * std::sqrt(norms[2 * (size_t)k + 1]);
        ps.residual[(size_t)k] = den > 0.0 ? std::sqrt(norms[2 * (size_t)k]) / den : 0.0;
    }
    info[3] = converged ? 1 : 0;
    ps.have = true;
    if (!converged)
        ctx->err = std::string(fn) + " stopped at the cap of " + std::to_string((int)max_outer) + " outer steps above the tolerance: last iterate returned";
    return MAG_OK;
}

// the argument checks both passes share, behind the null checks: sizes and tolerances; *q: the subspace with its default
int subspace_args_refused(mag_ctx *ctx, const char *fn, int32_t p, int32_t subspace, int32_t max_outer, double tol, double cg_tol, int32_t *q)
{
    if (p < 1) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: modes = %d: at least one mode", fn, (int)p);
    *q = subspace != 0 ? subspace : std::min(2 * p, p + 8);
    if (*q < p || *q > magk::kModalMaxQ)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: subspace = %d outside [modes = %d, %d]", fn, (int)*q, (int)p, magk::kModalMaxQ);
    if (max_outer < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: max_outer = %d is negative", fn, (int)max_outer);
    if (!(tol >= 0.0) || !std::isfinite(tol) || !(cg_tol >= 0.0) || !std::isfinite(cg_tol))
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: tol %g / cg_tol %g is negative or not finite", fn, tol, cg_tol);
    return MAG_OK;
}

// the results of a pass to the caller: values, residuals, shapes
int subspace_download(mag_ctx *ctx, const SubspacePass &ps, int32_t memory, double *values_out, double *residual_out, double *shapes_out)
{
    const int32_t p = ps.info[0];
    const auto [kind, hkind] = out_kinds(memory);
    hipStream_t s = ctx->stream;
    if (values_out) HIPCHK(hipMemcpyAsync(values_out, ps.lambda.data(), 8 * (size_t)p, hkind, s));
    if (residual_out) HIPCHK(hipMemcpyAsync(residual_out, ps.residual.data(), 8 * (size_t)p, hkind, s));
    if (shapes_out) HIPCHK(hipMemcpyAsync(shapes_out, ps.x.p, 16 * (size_t)ctx->N * (size_t)p, kind, s));
    return MAG_OK;
}

} // namespace

int mag_run_modal(mag_ctx *ctx, const mag_modal_options *mo)
{
    const char *fn = "mag_run_modal";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, fn);
    if (!mo) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_modal: null options");
    int32_t q = 0;
    if (int rc = subspace_args_refused(ctx, fn, mo->modes, mo->subspace, mo->max_outer, mo->tol, mo->cg_tol, &q)) return rc;
    if (int rc = mass_refused(ctx, fn, mo->density)) return rc;
    if (int rc = enter(ctx)) return rc;
    hipStream_t s = ctx->stream;
    SubspaceProblem sp = {fn, ctx->modal, mo->modes, q, mo->max_outer != 0 ? mo->max_outer : 50, mo->tol != 0.0 ? mo->tol : 1e-10,
                          mo->cg_tol != 0.0 ? mo->cg_tol : 1e-10, {}, {}, {}, {}};
    sp.second = [&](const magk::SensMesh &mesh, int32_t count, const double *x, double *y) -> int {
        magk::MassBatch mb;
        if (int rc = mass_batch(ctx, mo->density, mo->lumped, 1, count, x, y, mb)) return rc;
        magk::mass_apply(mesh, mb, s);
        return MAG_OK;
    };
    sp.ritz = [&](int32_t step, const double *A, const double *B, double *lambda, double *Q) -> int {
        int pivot = -1;
        double least = 0.0;
        const int eig = magh::sym_def_eig(q, A, B, lambda, Q, &pivot, &least);
        return ritz_status(ctx, fn, step, eig, pivot, least, "");
    };
    return subspace_iteration(ctx, sp);
}

int mag_download_modal(mag_ctx *ctx, mag_modal_result *o)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "null modal result");
    if (int rc = memory_refused(ctx, o->memory, "mag_download_modal")) return rc;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "modal analysis runs on one GPU: this context has a communicator of %d ranks", ctx->comm.nranks);
    if (!ctx->have_problem || !ctx->modal.have) return fail(ctx, MAG_ERR_STATE, "mag_download_modal before a completed mag_run_modal");
    if (int rc = enter(ctx)) return rc;
    const int32_t p = ctx->modal.info[0];
    hipStream_t s = ctx->stream;
    std::vector<double> freq((size_t)p);
    for (int32_t k = 0; k < p; ++k) freq[(size_t)k] = std::sqrt(ctx->modal.lambda[(size_t)k]) / (2.0 * M_PI);
    if (o->frequency_out) HIPCHK(hipMemcpyAsync(o->frequency_out, freq.data(), 8 * (size_t)p, out_kinds(o->memory).host, s));
    if (int rc = subspace_download(ctx, ctx->modal, o->memory, o->lambda_out, o->residual_out, o->shapes_out)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int mag_get_modal_info(const mag_ctx *ctx, int32_t info[8])
{
    if (!ctx || !info || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->have_problem || !ctx->modal.have) return MAG_ERR_STATE;
    for (int k = 0; k < 8; ++k) info[k] = ctx->modal.info[k];
    return MAG_OK;
}

int mag_get_modal_stats(const mag_ctx *ctx, int32_t j, mag_stats *st)
{
    if (!ctx || !st || j < 0 || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->have_problem || !ctx->modal.have) return MAG_ERR_STATE;
    return member_stats(ctx->modal.set, j, st);
}

int mag_apply_mass(mag_ctx *ctx, double density, int32_t lumped, const double *x, double *y, int32_t masked)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!x || !y) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_apply_mass: null vector");
    if (int rc = mass_refused(ctx, "mag_apply_mass", density)) return rc;
    if (int rc = enter(ctx)) return rc;
    if (int rc = ensure_full_order(ctx)) return rc;
    const int64_t N = ctx->N;
    const size_t vb = 16 * (size_t)N;
    hipStream_t s = ctx->stream;
    // (staged in the iteration's scratch vectors: the modes, like every other result, stay as they are)
    HIPCHK(ctx->modal.w.reserve(vb));
    HIPCHK(ctx->modal.y2.reserve(vb));
    magk::SensMesh mesh;
    magk::MassBatch mb;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->modal.w.p, x, vb, hipMemcpyHostToDevice, s));
    if (masked) magk::mask_vectors(ctx->uknown.as<uint8_t>(), N, 1, ctx->modal.w.as<double>(), s);
    if (int rc = mass_batch(ctx, density, lumped, masked, 1, ctx->modal.w.as<double>(), ctx->modal.y2.as<double>(), mb)) return rc;
    magk::mass_apply(mesh, mb, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(y, ctx->modal.y2.p, vb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// ---- linearised buckling (buckling.hip): the driver above with S = -K_G(sigma(u0)) and the pencil's Ritz step ----
namespace {

magk::Pattern transient_pattern(const mag_ctx *ctx); // (with the transient pass, below)

// the checks mag_run_buckling, mag_apply_geometric and mag_assemble_geometric share, before any HIP call: the context and the
// solved member whose solution is the prestress
int prestress_refused(mag_ctx *ctx, const char *fn, int32_t set, int32_t member)
{
    if (set != MAG_SET_RUN && set != MAG_SET_CASES)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: set %d: the prestress is a member of MAG_SET_RUN or MAG_SET_CASES", fn, (int)set);
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: buckling analysis runs on one GPU: this context has a communicator of %d ranks", fn, ctx->comm.nranks);
    const bool ran = set == MAG_SET_RUN ? ctx->have_run : ctx->cases.have_run;
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "%s before mag_upload", fn);
    if (!ran) return fail(ctx, MAG_ERR_STATE, "%s before a completed %s", fn, kSetRun[set]);
    const int32_t count = set == MAG_SET_RUN ? 1 : ctx->cases.count;
    if (member < 0 || member >= count) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: member %d outside the set's %d", fn, (int)member, (int)count);
    return MAG_OK;
}

// the solved member's displacements (2N, caller numbering, on the device), copied into bk_u0: nothing that runs later moves them
int prestress_copy(mag_ctx *ctx, int32_t set, int32_t member)
{
    const size_t vb = 16 * (size_t)ctx->N;
    const char *u = set == MAG_SET_RUN ? ctx->u.as<char>() : ctx->cases.u.as<char>() + vb * (size_t)member;
    HIPCHK(ctx->bk_u0.reserve(vb));
    HIPCHK(hipMemcpyAsync(ctx->bk_u0.p, u, vb, hipMemcpyDeviceToDevice, ctx->stream));
    return MAG_OK;
}

} // namespace

int mag_run_buckling(mag_ctx *ctx, const mag_buckling_options *bo)
{
    const char *fn = "mag_run_buckling";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, fn);
    if (!bo) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null options", fn);
    int32_t q = 0;
    if (int rc = subspace_args_refused(ctx, fn, bo->modes, bo->subspace, bo->max_outer, bo->tol, bo->cg_tol, &q)) return rc;
    if (int rc = prestress_refused(ctx, fn, bo->set, bo->member)) return rc;
    if (int rc = enter(ctx)) return rc;
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N;
    const int32_t p = bo->modes;
    SubspacePass &ps = ctx->buckling;
    ps.have = false;
    if (int rc = prestress_copy(ctx, bo->set, bo->member)) return rc;
    const double *u0 = ctx->bk_u0.as<double>();
    const auto no_stress = [&](const char *what, int32_t j) {
        return fail(ctx, MAG_ERR_STATE, "%s: the prestress vanishes (%s of start vector %d is not positive): member %d of set %d carries no stress", fn,
                    what, (int)j, (int)bo->member, (int)bo->set);
    };
    SubspaceProblem sp = {fn, ps, p, q, bo->max_outer != 0 ? bo->max_outer : 50, bo->tol != 0.0 ? bo->tol : 1e-10,
                          bo->cg_tol != 0.0 ? bo->cg_tol : 1e-10, {}, {}, {}, {}};
    sp.second = [&](const magk::SensMesh &mesh, int32_t count, const double *x, double *y) -> int {
        magk::GeomBatch gb;
        if (int rc = geometric_batch(ctx, u0, -1.0, 1, count, x, y, gb)) return rc;
        HIPCHK(magk::geometric_apply(mesh, gb, s));
        return MAG_OK;
    };
    sp.start = [&](const double *Y, double *d_norms) -> int { // (a right-hand side of zero is no system to solve)
        std::vector<double> norms(2 * (size_t)q);
        magk::residual_norms(Y, Y, N, q, ps.part.as<double>(), d_norms, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(norms.data(), d_norms, 8 * norms.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int32_t j = 0; j < q; ++j)
            if (!(norms[2 * (size_t)j] > 0.0)) return no_stress("|K_G x|", j);
        return MAG_OK;
    };
    sp.first_gram = [&](const double *A) -> int {
        for (int32_t j = 0; j < q; ++j)
            if (!(A[(size_t)j * q + j] > 0.0)) return no_stress("A_jj", j);
        return MAG_OK;
    };
    sp.ritz = [&](int32_t step, const double *A, const double *B, double *lambda, double *Q) -> int {
        int pivot = -1;
        double least = 0.0, mu[magh::kEigMaxN];
        const int eig = magh::sym_pencil_eig(q, A, B, mu, Q, &pivot, &least);
        if (int rc = ritz_status(ctx, fn, step, eig, pivot, least,
                                 ": a K_G of rank below the subspace's size causes it, a smaller subspace helps"))
            return rc;
        for (int32_t k = 0; k < p; ++k)
            if (!(std::fabs(mu[k]) > magh::kEigPivotTol * std::fabs(mu[0])))
                return fail(ctx, MAG_ERR_NOT_CONVERGED,
                            "%s: outer step %d: fewer than %d buckling modes exist (|mu_%d| = %.3g against |mu_1| = %.3g, refused at or below %.3g of it)",
                            fn, (int)step + 1, (int)p, (int)k + 1, std::fabs(mu[k]), std::fabs(mu[0]), magh::kEigPivotTol);
        for (int32_t k = 0; k < q; ++k) lambda[k] = 1.0 / mu[k]; // (a guard vector's mu may be 0: its factor is infinite and unused)
        return MAG_OK;
    };
    sp.k_normalise = true;
    if (int rc = subspace_iteration(ctx, sp)) return rc;
    for (int32_t k = 0; k < p; ++k) ps.info[7] += ps.lambda[(size_t)k] > 0.0 ? 1 : 0;
    return MAG_OK;
}

int mag_download_buckling(mag_ctx *ctx, mag_buckling_result *o)
{
    const char *fn = "mag_download_buckling";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "null buckling result");
    if (int rc = memory_refused(ctx, o->memory, fn)) return rc;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: buckling analysis runs on one GPU: this context has a communicator of %d ranks", fn, ctx->comm.nranks);
    if (!ctx->have_problem || !ctx->buckling.have) return fail(ctx, MAG_ERR_STATE, "%s before a completed mag_run_buckling", fn);
    if (int rc = enter(ctx)) return rc;
    if (int rc = subspace_download(ctx, ctx->buckling, o->memory, o->load_factor_out, o->residual_out, o->shapes_out)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MAG_OK;
}

int mag_get_buckling_info(const mag_ctx *ctx, int32_t info[8])
{
    if (!ctx || !info || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->have_problem || !ctx->buckling.have) return MAG_ERR_STATE;
    for (int k = 0; k < 8; ++k) info[k] = ctx->buckling.info[k];
    return MAG_OK;
}

int mag_get_buckling_stats(const mag_ctx *ctx, int32_t j, mag_stats *st)
{
    if (!ctx || !st || j < 0 || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->have_problem || !ctx->buckling.have) return MAG_ERR_STATE;
    return member_stats(ctx->buckling.set, j, st);
}

int mag_apply_geometric(mag_ctx *ctx, int32_t set, int32_t member, const double *x, double *y, int32_t masked)
{
    const char *fn = "mag_apply_geometric";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, fn);
    if (!x || !y) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null vector", fn);
    if (int rc = prestress_refused(ctx, fn, set, member)) return rc;
    if (int rc = enter(ctx)) return rc;
    if (int rc = ensure_full_order(ctx)) return rc;
    const int64_t N = ctx->N;
    const size_t vb = 16 * (size_t)N;
    hipStream_t s = ctx->stream;
    // (staged in the iteration's scratch vectors: the shapes, like every other result, stay as they are)
    HIPCHK(ctx->buckling.w.reserve(vb));
    HIPCHK(ctx->buckling.y2.reserve(vb));
    magk::SensMesh mesh;
    magk::GeomBatch gb;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    if (int rc = prestress_copy(ctx, set, member)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->buckling.w.p, x, vb, hipMemcpyHostToDevice, s));
    if (masked) magk::mask_vectors(ctx->uknown.as<uint8_t>(), N, 1, ctx->buckling.w.as<double>(), s);
    if (int rc = geometric_batch(ctx, ctx->bk_u0.as<double>(), 1.0, masked, 1, ctx->buckling.w.as<double>(), ctx->buckling.y2.as<double>(), gb))
        return rc;
    HIPCHK(magk::geometric_apply(mesh, gb, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(y, ctx->buckling.y2.p, vb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int mag_assemble_geometric(mag_ctx *ctx, int32_t set, int32_t member, double *values_out, int32_t memory)
{
    const char *fn = "mag_assemble_geometric";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, fn);
    if (!values_out) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null values_out", fn);
    if (int rc = memory_refused(ctx, memory, fn)) return rc;
    if (int rc = prestress_refused(ctx, fn, set, member)) return rc;
    if (ctx->opt.assemble_csr == 0) return fail(ctx, MAG_ERR_STATE, "%s: needs K's pattern: this context has assemble_csr = 0", fn);
    if (int rc = enter(ctx)) return rc;
    if (int rc = ensure_csr(ctx)) return rc;
    hipStream_t s = ctx->stream;
    const size_t ab = 32 * (size_t)ctx->nb;
    HIPCHK(ctx->bk_kg.reserve(ab));
    magk::SensMesh mesh;
    MemberView mv;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    if (int rc = member_view(ctx, MAG_SET_RUN, mv)) return rc; // (the uploaded material, on the device)
    if (int rc = prestress_copy(ctx, set, member)) return rc;
    magk::geometric_values(mesh, transient_pattern(ctx), ctx->xy.as<double>(), mv.mat, ctx->bk_u0.as<double>(), ctx->bk_kg.as<double>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(values_out, ctx->bk_kg.p, ab, out_kinds(memory).dev, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// ---- transient dynamics (transient.hip): Newmark time stepping of the uploaded part.  The driver owns the buffers, builds the
// mass and the effective matrix in K's pattern, prepares the solver's copy of it once per system (the a_0 system, then the
// step's) and enqueues every step on the context's stream: the host reads the CG's convergence polls and nothing else.  The
// solver (ImplicitSolver), its table (ptab) and the device checks' scratch (chk_*) are shared with the two Newton passes ----
namespace {

constexpr int kTransientPoll = 8; // launches per poll block behind a solve's first block (even: the parity restarts per block)

// The inner solves of the implicit passes (mag_run_transient, mag_run_newton, mag_run_transient_tl): a matrix in kval's layout,
// the block-row table and the inverse blocks (ptab; or the reduced system of the CSR phase), and the poll scheme, in one
// place.  The solves run under MAG_STOP_REL with cg_tol, silently, launched one by one (the pass chooses the poll's block
// length per solve) and without a cost history; the context's options, statistics and the CSR phase's counts are as they were
// once the object goes, on every exit path.
struct ImplicitSolver {
    // mag_*_options.cg: the fused block-row CG (kind: its preconditioner) or the CSR phase's
    struct Choice {
        bool fused;
        int kind;
    };
    static int choose(mag_ctx *ctx, const char *fn, int32_t cg, Choice *c)
    {
        c->fused = cg == 0 ? ctx->use_lds : cg <= 3;
        if (c->fused && !ctx->use_lds)
            return fail(ctx, MAG_ERR_STATE, "%s: cg = %d needs the tile-local tables, which this context does not build (op_variant, or a tile beyond the LDS)",
                        fn, (int)cg);
        c->kind = !c->fused ? 0 : (cg == 0 ? 2 : cg - 1);
        return MAG_OK;
    }

    mag_ctx *ctx;
    const char *fn;
    const bool fused;
    const int kind;
    const mag_options opt;
    const mag_stats stats;
    const double best_cost;
    const long long best_iter;
    const int64_t nf, nz_ff;
    const int32_t cg_kernel;
    FieldTable tab;
    FieldSystem sys = {};
    long long prev = -1; // the iterations of the previous solve

    ImplicitSolver(mag_ctx *c, const char *fn_, Choice ch, double cg_tol)
        : ctx(c), fn(fn_), fused(ch.fused), kind(ch.kind), opt(c->opt), stats(c->stats), best_cost(c->best_cost), best_iter(c->best_iter), nf(c->nf),
          nz_ff(c->nz_ff), cg_kernel(c->cg_kernel), tab(pass_table(c))
    {
        ctx->opt.stop_mode = MAG_STOP_REL;
        ctx->opt.tol = cg_tol;
        ctx->opt.verbose = 0;
        ctx->opt.use_graph = 0;
        ctx->opt.history_len = 0;
    }
    ImplicitSolver(const ImplicitSolver &) = delete;
    ~ImplicitSolver()
    {
        ctx->opt = opt;
        ctx->stats = stats;
        ctx->best_cost = best_cost;
        ctx->best_iter = best_iter;
        ctx->nf = nf;
        ctx->nz_ff = nz_ff;
        ctx->cg_kernel = cg_kernel;
        ctx->tr_first_block = 0;
    }
    // the table of the order and the pattern held now
    int init()
    {
        if (!fused) return MAG_OK;
        if (int rc = build_field_table(ctx, tab)) return rc;
        sys = {tab.meta.as<magk::FieldTileMeta>(), tab.slot.as<uint16_t>(), tab.val.as<double2>(), nullptr, nullptr, tab.total,
               magk::field_cg_grid(ctx->B, ctx->cap, ctx->T, kind != 0)};
        return MAG_OK;
    }
    // the solver's copy of the matrix in val: the gathered block rows and the inverse blocks, or the reduced system
    int system(const double *val)
    {
        if (!fused) return build_reduced(ctx, true, val, false);
        if (int rc = field_values(ctx, tab, val, kind, ctx->ptab.minv, ctx->ptab.hminv)) return rc;
        sys.minvP = kind ? ctx->ptab.minv.as<float4>() : nullptr;
        sys.halo_minv = kind ? ctx->ptab.hminv.as<float4>() : nullptr;
        return MAG_OK;
    }
    // A_FF x_F = rhs_F from zero, x_P = xP.  The poll's first block: the previous solve's iteration count + 2 (a launch judges the
    // iterate of the one before), rounded up to even -- the context's check_every for the first solve --, then blocks of
    // kTransientPoll.  Launches behind convergence are no-ops: the results do not depend on it.  before / after: events recorded
    // around the CG itself (behind the move into the solver's numbering, in front of the move back), or null.  The statistics of
    // the solve are the context's (ctx->stats) on return; a solve that broke down is refused, named by `where` (a format and its
    // arguments: "step %d")
    __attribute__((format(printf, 7, 8))) int solve(const double *rhs, const double *xP, double *x, hipEvent_t before, hipEvent_t after,
                                                    const char *where, ...)
    {
        hipStream_t s = ctx->stream;
        const int64_t N = ctx->N;
        const uint8_t *known = ctx->uknown.as<uint8_t>();
        long long G = prev < 0 ? opt.check_every : std::min<long long>(prev + 2, 4096);
        G += G & 1;
        ctx->tr_first_block = (int32_t)std::max<long long>(G, 2);
        ctx->opt.check_every = kTransientPoll;
        if (fused) {
            magk::to_hilbert(rhs, ctx->iperm.as<int32_t>(), known, 0, N, ctx->bP.as<double>(), s);
            if (before) HIPCHK(hipEventRecord(before, s));
            if (int rc = cg_phase_field(ctx, sys)) return rc;
            if (after) HIPCHK(hipEventRecord(after, s));
            magk::scatter_back(ctx->x.as<double>(), ctx->perm.as<uint32_t>(), known, xP, N, x, s);
        } else {
            magk::compact_free(rhs, ctx->fidx.as<int32_t>(), known, 2 * N, ctx->b_ff.as<double>(), s);
            if (before) HIPCHK(hipEventRecord(before, s));
            if (int rc = cg_phase_csr(ctx, true, xP, x)) return rc;
            if (after) HIPCHK(hipEventRecord(after, s));
        }
        HIPCHK(hipGetLastError());
        prev = ctx->stats.iterations;
        if (ctx->stats.breakdown) {
            char at[64];
            va_list ap;
            va_start(ap, where);
            vsnprintf(at, sizeof at, where, ap);
            va_end(ap);
            return fail(ctx, MAG_ERR_NOT_CONVERGED, "%s: %s: the solve broke down (non-finite residual after %lld iterations)", fn, at, prev);
        }
        return MAG_OK;
    }
};

// the contexts the pass does not run on, before any HIP call
int transient_refused(mag_ctx *ctx, const char *fn)
{
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: transient dynamics run on one GPU: this context has a communicator of %d ranks", fn, ctx->comm.nranks);
    if (ctx->opt.assemble_csr == 0) return fail(ctx, MAG_ERR_STATE, "%s: needs the assembled K: this context has assemble_csr = 0", fn);
    if (ctx->opt.precision == 1) return fail(ctx, MAG_ERR_STATE, "%s: not available with precision = 1 (the fp32 leg is matrix-free)", fn);
    if (ctx->field_on) return field_refuses(ctx, fn);
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "%s before mag_upload", fn);
    return MAG_OK;
}

// the uploads the context's material law does not cover, before any device work (the six total-Lagrangian entry points)
int law_refused(mag_ctx *ctx, const char *fn)
{
    if (ctx->law == MAG_LAW_NEO_HOOKE && !(ctx->nu < 0.5 && ctx->nu > -1.0))
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: nu = %g is outside (-1, 0.5): MAG_LAW_NEO_HOOKE needs a compressible material", fn, ctx->nu);
    return MAG_OK;
}

magk::Pattern transient_pattern(const mag_ctx *ctx) { return {ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), ctx->N, ctx->nb}; }

// K assembled, and M in its pattern (tr_mval); room for A (tr_aval)
int transient_matrices(mag_ctx *ctx, double density, int32_t lumped)
{
    if (int rc = ensure_csr(ctx)) return rc;
    HIPCHK(ctx->tr_mval.reserve(8 * (size_t)ctx->nb));
    HIPCHK(ctx->tr_aval.reserve(32 * (size_t)ctx->nb));
    magk::mass_pattern(transient_pattern(ctx), ctx->perm.as<uint32_t>(), ctx->inc_off.as<int32_t>(), ctx->inc.as<uint32_t>(),
                       ctx->conn.as<int32_t>(), ctx->xy.as<double>(), density * ctx->thick, lumped ? 1 : 0, ctx->tr_mval.as<double>(),
                       ctx->stream);
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

// ---- what mag_run_transient and mag_run_explicit share: the set-up of a stepping pass on the host

// the option fields both passes have
struct StepOptions {
    int32_t steps, snapshot_every, num_probes;
    const int32_t *probes;
    int32_t memory, resume;
    const double *amplitude, *u0, *v0;
};

// the tail of the argument checks, behind the pass's own: the records, the context, the resume rule; enters the context
int step_args_tail(mag_ctx *ctx, const char *fn, const StepOptions &o)
{
    if (o.snapshot_every < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: snapshot_every = %d is negative", fn, (int)o.snapshot_every);
    if (o.num_probes < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: num_probes = %d is negative", fn, (int)o.num_probes);
    if (o.num_probes > 0 && !o.probes) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: num_probes = %d with null probes", fn, (int)o.num_probes);
    if (int rc = memory_refused(ctx, o.memory, fn)) return rc;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: transient dynamics run on one GPU: this context has a communicator of %d ranks", fn, ctx->comm.nranks);
    if (o.resume && (o.u0 || o.v0)) return fail(ctx, MAG_ERR_STATE, "%s: resume starts from the previous run's state: u0 / v0 must be NULL", fn);
    if (o.resume && !(ctx->have_problem && ctx->tr_have)) return fail(ctx, MAG_ERR_STATE, "%s: resume without a completed run of the pass", fn);
    if (int rc = transient_refused(ctx, fn)) return rc;
    return enter(ctx);
}

// the orientation kernel's word (all ones: nothing found), refused
int clockwise_refused(mag_ctx *ctx, const char *fn, unsigned long long clockwise)
{
    if (clockwise == ~0ull) return MAG_OK;
    return fail(ctx, MAG_ERR_BAD_ARGS,
                "%s: element %lld has a signed area <= 0 (the stiffness carries the signed area: the pass needs counter-clockwise elements)", fn,
                (long long)clockwise);
}

// What mag_internal_force, mag_assemble_tangent and mag_assemble_effective_tangent share: one evaluation at a caller's state u,
// in scratch that holds no result of the context (ev_u, ev_words).  enqueue(d_u, d_words) launches the kernel, which writes
// `out`; the elements' orientation is checked in front of it, `bytes` of `out` go to the caller behind it, *h receives the words
struct EvalWords {
    unsigned long long clockwise; // the first element of signed area <= 0
    int32_t inverted, pad;
    double W;
};
int evaluate_at(mag_ctx *ctx, const char *fn, const double *u, int32_t memory, const std::function<void(const double *, EvalWords *)> &enqueue,
                const DevBuf &out, size_t bytes, void *dst, EvalWords *h)
{
    hipStream_t s = ctx->stream;
    const size_t vb = 16 * (size_t)ctx->N;
    HIPCHK(ctx->ev_u.reserve(vb));
    HIPCHK(ctx->ev_words.reserve(sizeof(EvalWords)));
    EvalWords *d = ctx->ev_words.as<EvalWords>();
    HIPCHK(hipMemsetAsync(&d->inverted, 0, 8, s));
    HIPCHK(hipMemcpyAsync(ctx->ev_u.p, u, vb, in_kind_of(memory), s));
    magk::orientation(ctx->xy.as<double>(), ctx->conn.as<int32_t>(), ctx->N, ctx->E, &d->clockwise, s);
    enqueue(ctx->ev_u.as<double>(), d);
    HIPCHK(hipGetLastError());
    *h = {~0ull, 0, 0, 0.0};
    HIPCHK(hipMemcpyAsync(h, d, sizeof(EvalWords), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = clockwise_refused(ctx, fn, h->clockwise)) return rc;
    HIPCHK(hipMemcpyAsync(dst, out.p, bytes, out_kinds(memory).dev, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// The 16 bytes of chk_words.  The device checks write two words (all ones: nothing found); once those are read back, the explicit
// pass keeps its flags in the same bytes: the finite flag at byte 0, the inverted-element flag at byte 8
struct StepWords {
    union {
        unsigned long long clockwise; // the first element of signed area <= 0
        int32_t not_finite;
    };
    union {
        unsigned long long bad_probe; // the first probe outside [0, 2N)
        int32_t inverted;
    };
};
static_assert(sizeof(StepWords) == 16 && offsetof(StepWords, bad_probe) == 8 && offsetof(StepWords, inverted) == 8, "chk_words' layout");

// the checks that need the device, enqueued: the elements' orientation, the probes (uploaded into chk_probes); *h receives the
// words once the stream is synchronised
int step_checks_enqueue(mag_ctx *ctx, const StepOptions &o, StepWords *h)
{
    hipStream_t s = ctx->stream;
    const int32_t np = o.num_probes;
    HIPCHK(ctx->chk_words.reserve(sizeof(StepWords)));
    HIPCHK(ctx->chk_probes.reserve(4 * (size_t)std::max(np, 1)));
    h->clockwise = h->bad_probe = ~0ull;
    StepWords *d = ctx->chk_words.as<StepWords>();
    if (np > 0) HIPCHK(hipMemcpyAsync(ctx->chk_probes.p, o.probes, 4 * (size_t)np, in_kind_of(o.memory), s));
    magk::orientation(ctx->xy.as<double>(), ctx->conn.as<int32_t>(), ctx->N, ctx->E, &d->clockwise, s);
    magk::check_probes(ctx->chk_probes.as<int32_t>(), np, 2 * ctx->N, &d->bad_probe, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, d, sizeof(StepWords), hipMemcpyDeviceToHost, s));
    return MAG_OK;
}

// ... and reported, behind the synchronise
int step_checks_report(mag_ctx *ctx, const char *fn, const StepWords &h)
{
    if (int rc = clockwise_refused(ctx, fn, h.clockwise)) return rc;
    if (h.bad_probe != ~0ull)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: probes[%lld] is outside [0, %lld)", fn, (long long)h.bad_probe, (long long)(2 * ctx->N));
    return MAG_OK;
}

// the buffers of a run of `rows` record rows, `amp_n` amplitudes and `snaps` snapshots: the records first, against the memory
// that is free now; the state (a resumed run finds it there), the work vectors, tr_zero zeroed
int step_buffers(mag_ctx *ctx, const char *fn, int32_t steps, size_t rows, size_t amp_n, size_t snaps, int32_t np, bool resume)
{
    const size_t vb = 16 * (size_t)ctx->N;
    const size_t probe_b = 3 * 8 * rows * (size_t)std::max(np, 1), energy_b = 3 * 8 * rows, snap_b = snaps * vb;
    {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        auto more = [](const DevBuf &b, size_t want) { return want > b.cap ? want + (want >> 4) + 256 : (size_t)0; };
        const size_t need = more(ctx->tr_probe, probe_b) + more(ctx->tr_energy, energy_b) + more(ctx->tr_snap, snap_b) + more(ctx->tr_amp, 8 * amp_n);
        if (need > free_b)
            return fail(ctx, MAG_ERR_TOO_LARGE, "%s: the records of %d steps need %zu bytes of device memory, %zu are free", fn, (int)steps, need, free_b);
    }
    HIPCHK(ctx->tr_probe.reserve(probe_b));
    HIPCHK(ctx->tr_energy.reserve(energy_b));
    HIPCHK(ctx->tr_snap.reserve(std::max<size_t>(snap_b, 8)));
    HIPCHK(ctx->tr_amp.reserve(8 * amp_n));
    HIPCHK(ctx->tr_part.reserve(8 * 3 * (size_t)magk::kSensBlocks));
    for (DevBuf *b : {&ctx->tr_u, &ctx->tr_v, &ctx->tr_a}) {
        if (resume && b->cap < vb) return fail(ctx, MAG_ERR_STATE, "%s: resume without the state of a completed run", fn);
        HIPCHK(b->reserve(vb));
    }
    for (DevBuf *b : {&ctx->tr_ut, &ctx->tr_vt, &ctx->tr_rhs, &ctx->tr_zero, &ctx->tr_f, &ctx->tr_ku, &ctx->tr_mv}) HIPCHK(b->reserve(vb));
    HIPCHK(hipMemsetAsync(ctx->tr_zero.p, 0, vb, ctx->stream));
    return MAG_OK;
}

// the inputs on the device: the amplitude in tr_amp (ones where none is given; a resumed run's row 0 carries amp_first, the load
// of the state it resumes), u0 / v0 in tr_in (null where none is given); synchronises (the host's copies are done with)
struct StepInputs {
    const double *d_u0, *d_v0;
    double amp_last; // amplitude[steps]
};
int step_inputs(mag_ctx *ctx, const StepOptions &o, size_t amp_n, double amp_first, StepInputs *in)
{
    hipStream_t s = ctx->stream;
    const hipMemcpyKind in_kind = in_kind_of(o.memory);
    const size_t vb = 16 * (size_t)ctx->N;
    std::vector<double> ones;
    double *d_amp = ctx->tr_amp.as<double>();
    if (o.amplitude) {
        HIPCHK(hipMemcpyAsync(d_amp, o.amplitude, 8 * amp_n, in_kind, s));
    } else {
        ones.assign(amp_n, 1.0);
        HIPCHK(hipMemcpyAsync(d_amp, ones.data(), 8 * amp_n, hipMemcpyHostToDevice, s));
    }
    if (o.resume) HIPCHK(hipMemcpyAsync(d_amp, &amp_first, 8, hipMemcpyHostToDevice, s));
    *in = {nullptr, nullptr, 1.0};
    HIPCHK(hipMemcpyAsync(&in->amp_last, d_amp + o.steps, 8, hipMemcpyDeviceToHost, s));
    if (o.u0 || o.v0) {
        HIPCHK(ctx->tr_in.reserve(2 * vb));
        if (o.u0) {
            HIPCHK(hipMemcpyAsync(ctx->tr_in.p, o.u0, vb, in_kind, s));
            in->d_u0 = ctx->tr_in.as<double>();
        }
        if (o.v0) {
            HIPCHK(hipMemcpyAsync(ctx->tr_in.as<char>() + vb, o.v0, vb, in_kind, s));
            in->d_v0 = ctx->tr_in.as<double>() + 2 * ctx->N;
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// the state and the probe records of a run of `rows` rows, in the context's buffers
magk::NewmarkState newmark_state(const mag_ctx *ctx, size_t rows, int32_t np)
{
    magk::NewmarkState st = {};
    st.n2 = 2 * ctx->N;
    st.u = ctx->tr_u.as<double>();
    st.v = ctx->tr_v.as<double>();
    st.a = ctx->tr_a.as<double>();
    st.ut = ctx->tr_ut.as<double>();
    st.vt = ctx->tr_vt.as<double>();
    st.known = ctx->uknown.as<uint8_t>();
    st.u_in = ctx->uin.as<double>();
    st.num_probes = np;
    st.probes = ctx->chk_probes.as<int32_t>();
    st.probe_u = ctx->tr_probe.as<double>();
    st.probe_v = st.probe_u + rows * (size_t)np;
    st.probe_a = st.probe_v + rows * (size_t)np;
    return st;
}

// tr_rhs = (amplitude[amp_at] f - alpha M xv - K (x + eta xv))_F, 0 on P: the right-hand side of a_0 (x, xv = u, v) and of a step
// (ut, vt)
void damped_rhs(mag_ctx *ctx, const magk::NewmarkState &st, const double *x, const double *xv, double alpha, double eta, int64_t amp_at)
{
    magk::PatternApply r = {};
    r.kval = ctx->kval.as<double>(), r.mval = ctx->tr_mval.as<double>(), r.xa = x, r.ca = 1.0, r.xb = eta != 0.0 ? xv : nullptr, r.cb = eta;
    r.xc = alpha != 0.0 ? xv : nullptr, r.cc = alpha;
    r.kind = 1, r.known = st.known, r.f = ctx->fin.as<double>(), r.amplitude = ctx->tr_amp.as<double>(), r.amp_at = amp_at;
    r.y = ctx->tr_rhs.as<double>();
    magk::pattern_apply(transient_pattern(ctx), r, ctx->stream);
}

// tr_f = the reactions of the final state: K (u + eta v) + M (a + alpha v) on P, amplitude[steps] f on F
void linear_reactions(mag_ctx *ctx, const magk::NewmarkState &st, double alpha, double eta, int64_t steps)
{
    magk::PatternApply r = {};
    r.kval = ctx->kval.as<double>(), r.mval = ctx->tr_mval.as<double>(), r.xa = st.u, r.ca = 1.0, r.xb = eta != 0.0 ? st.v : nullptr, r.cb = eta;
    r.xc = st.a, r.cc = 1.0, r.xd = alpha != 0.0 ? st.v : nullptr, r.cd = alpha;
    r.kind = 2, r.known = st.known, r.f = ctx->fin.as<double>(), r.amplitude = ctx->tr_amp.as<double>(), r.amp_at = steps;
    r.y = ctx->tr_f.as<double>();
    magk::pattern_apply(transient_pattern(ctx), r, ctx->stream);
}

// energy row `row` of the state under amplitude[amp_at]: T = 1/2 v.Mv, W = 1/2 u.Ku, P = amplitude[amp_at] f.u_F
void linear_energy_row(mag_ctx *ctx, const magk::NewmarkState &st, int64_t row, int64_t amp_at)
{
    magk::PatternApply e = {};
    e.kval = ctx->kval.as<double>(), e.mval = ctx->tr_mval.as<double>(), e.xa = st.u, e.ca = 1.0, e.xc = st.v, e.cc = 1.0;
    e.y = ctx->tr_rhs.as<double>(), e.ku = ctx->tr_ku.as<double>(), e.mv = ctx->tr_mv.as<double>();
    magk::pattern_apply(transient_pattern(ctx), e, ctx->stream);
    magk::newmark_energies(st, e.ku, e.mv, ctx->fin.as<double>(), ctx->tr_amp.as<double>(), amp_at, ctx->tr_part.as<double>(),
                           ctx->tr_energy.as<double>() + 3 * row, ctx->stream);
}

// the mesh as the total-Lagrangian kernels read it in caller numbering
magk::TlMesh tl_mesh(const mag_ctx *ctx)
{
    magk::TlMesh m = {};
    m.N = ctx->N, m.E = ctx->E;
    m.perm = ctx->perm.as<uint32_t>(), m.inc_off = ctx->inc_off.as<int32_t>(), m.inc = ctx->inc.as<uint32_t>();
    m.conn = ctx->conn.as<int32_t>(), m.xy = ctx->xy.as<double2>();
    set_tl_material(ctx, m);
    return m;
}

// what the two fused step kernels share, but the step itself (in, out, dt, amp_at)
magk::StepFrame step_frame(const mag_ctx *ctx, double alpha)
{
    magk::StepFrame F = {};
    F.N = ctx->N, F.T = ctx->T, F.cap = ctx->cap;
    F.maskP = ctx->maskP.as<uint8_t>();
    F.halo_g = ctx->halo_g.as<int32_t>();
    F.uinP = ctx->ex_uin.as<double2>(), F.fP = ctx->ex_f.as<double2>(), F.massP = ctx->ex_mass.as<double>();
    F.amplitude = ctx->tr_amp.as<double>(), F.alpha = alpha;
    return F;
}

// the results of a completed run, but the pass's own info words and tr_iterations
void publish_steps(mag_ctx *ctx, const StepOptions &o, bool energies, size_t rows, size_t snaps, double t_start, double dt, double amp_last,
                   double dt_recorded, double dt_bound)
{
    ctx->tr_steps = o.steps;
    ctx->tr_num_probes = o.num_probes;
    ctx->tr_snaps = (int32_t)snaps;
    ctx->tr_energies = energies;
    ctx->tr_t0 = t_start;
    ctx->tr_t1 = t_start + (double)o.steps * dt;
    ctx->tr_amp_last = amp_last;
    ctx->tr_rows = (int64_t)rows;
    ctx->tr_dt = dt_recorded;
    ctx->tr_dt_bound = dt_bound;
    ctx->tr_have = true;
}

// ---- what the Newton loops of mag_run_newton and mag_run_transient_tl share on the host

// MAG_TUNE_*_TIMES (env: the variable): the n phases of every iteration between the events ctx->ev[0..n], summed over the run
struct PhaseTimer {
    mag_ctx *ctx;
    const char *path;
    const int n;
    double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    PhaseTimer(mag_ctx *c, const char *env, int phases) : ctx(c), path(getenv(env)), n(phases) {}
    bool on() const { return path && *path; }
    hipEvent_t event(int k) const { return on() ? ctx->ev[k] : nullptr; }
    int stamp(int k)
    {
        if (on()) HIPCHK(hipEventRecord(ctx->ev[k], ctx->stream));
        return MAG_OK;
    }
    // the iteration's phases, once event n has completed (wait: not behind a synchronise of the stream yet)
    int add(bool wait)
    {
        if (!on()) return MAG_OK;
        if (wait) HIPCHK(hipEventSynchronize(ctx->ev[n]));
        for (int ph = 0; ph < n; ++ph) {
            float t = 0.0f;
            HIPCHK(hipEventElapsedTime(&t, ctx->ev[ph], ctx->ev[ph + 1]));
            ms[ph] += t;
        }
        return MAG_OK;
    }
    __attribute__((format(printf, 2, 3))) void append(const char *fmt, ...)
    {
        FILE *tf = on() ? fopen(path, "a") : nullptr;
        if (!tf) return;
        va_list ap;
        va_start(ap, fmt);
        vfprintf(tf, fmt, ap);
        va_end(ap);
        fclose(tf);
    }
};

// the stop rule: |r_F| <= tol * ref, from the squares of the norms; ratio: what the records keep
struct NewtonStop {
    double ratio;
    bool converged;
};
inline NewtonStop newton_stop(double r2, double ref2, double tol)
{
    const double rn = std::sqrt(r2), ref = std::sqrt(ref2);
    return {ref > 0.0 ? rn / ref : (rn == 0.0 ? 0.0 : INFINITY), rn <= tol * ref};
}

// the warning of a run that stopped at the cap (what: "increment" / "step")
void newton_unconverged(std::string &msg, const char *fn, const char *what, int index, int cap, double ratio, int it, double tol)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s %d did not converge within %d iterations: |r_F| / ref = %.3e after iteration %d (tolerance %.3e)", fn, what, index,
             cap, ratio, it, tol);
    msg = buf;
}

} // namespace

void mag_default_transient_options(mag_transient_options *o)
{
    if (!o) return;
    *o = {};
    o->beta = 0.25;
    o->gamma = 0.5;
}

int mag_assemble_effective(mag_ctx *ctx, double c_K, double c_M, double density, int32_t lumped, double *values_out, int32_t memory)
{
    const char *fn = "mag_assemble_effective";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!values_out) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null values_out", fn);
    if (!std::isfinite(c_K) || !std::isfinite(c_M)) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: c_K %g / c_M %g is not finite", fn, c_K, c_M);
    if (int rc = need_pos(ctx, fn, {{"density", density}})) return rc;
    if (int rc = memory_refused(ctx, memory, fn)) return rc;
    if (int rc = transient_refused(ctx, fn)) return rc;
    if (int rc = enter(ctx)) return rc;
    if (int rc = transient_matrices(ctx, density, lumped)) return rc;
    hipStream_t s = ctx->stream;
    magk::effective_values(transient_pattern(ctx), ctx->kval.as<double>(), ctx->tr_mval.as<double>(), c_K, c_M, ctx->tr_aval.as<double>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(values_out, ctx->tr_aval.p, 32 * (size_t)ctx->nb, memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int mag_run_transient(mag_ctx *ctx, const mag_transient_options *o)
{
    const char *fn = "mag_run_transient";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null options", fn);
    if (o->steps < 1) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: steps = %d: at least one step", fn, (int)o->steps);
    if (int rc = need_pos(ctx, fn, {{"dt", o->dt}, {"density", o->density}})) return rc;
    if (int rc = need_nonneg(ctx, fn, {{"beta", o->beta}, {"gamma", o->gamma}, {"rayleigh_mass", o->rayleigh_mass},
                                       {"rayleigh_stiffness", o->rayleigh_stiffness}, {"cg_tol", o->cg_tol}}))
        return rc;
    if (o->cg < 0 || o->cg > 4) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: cg = %d outside 0..4", fn, (int)o->cg);
    const StepOptions so = {o->steps, o->snapshot_every, o->num_probes, o->probes, o->memory, o->resume, o->amplitude, o->u0, o->v0};
    if (int rc = step_args_tail(ctx, fn, so)) return rc;

    const bool resume = o->resume != 0, energies = o->energies != 0;
    const int32_t steps = o->steps, np = o->num_probes, se = o->snapshot_every;
    const double dt = o->dt, beta = o->beta, gamma = o->gamma, alpha = o->rayleigh_mass, eta = o->rayleigh_stiffness;
    const double cg_tol = o->cg_tol != 0.0 ? o->cg_tol : 1e-10;
    const double t_start = resume ? ctx->tr_t1 : 0.0;
    const double amp_first = ctx->tr_amp_last; // (a resumed run's row 0 carries the load of the state it resumes)
    ctx->tr_have = ctx->tt_have = false; // (a failure leaves no results of the pass)
    hipStream_t s = ctx->stream;

    if (int rc = transient_matrices(ctx, o->density, o->lumped)) return rc;
    if (int rc = reserve_cg(ctx)) return rc;
    const int64_t N = ctx->N, n2 = 2 * N;
    const magk::Pattern pat = transient_pattern(ctx);

    // ---- the checks that need the device: the elements' orientation, the probes
    StepWords words;
    if (int rc = step_checks_enqueue(ctx, so, &words)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = step_checks_report(ctx, fn, words)) return rc;

    ImplicitSolver::Choice choice;
    if (int rc = ImplicitSolver::choose(ctx, fn, o->cg, &choice)) return rc;

    // ---- the buffers, the inputs
    const size_t rows = (size_t)steps + 1, snaps = se > 0 ? (size_t)(steps / se) + 1 : 0;
    if (int rc = step_buffers(ctx, fn, steps, rows, rows, snaps, np, resume)) return rc;
    StepInputs in;
    if (int rc = step_inputs(ctx, so, rows, amp_first, &in)) return rc;
    const magk::NewmarkState st = newmark_state(ctx, rows, np);
    double *d_rhs = ctx->tr_rhs.as<double>(), *d_snap = ctx->tr_snap.as<double>();
    const double *d_k = ctx->kval.as<double>(), *d_m = ctx->tr_mval.as<double>();

    ImplicitSolver solver(ctx, fn, choice, cg_tol);
    if (int rc = solver.init()) return rc;
    // A = c_M M + c_K K and the solver's copy of it
    auto system = [&](double c_M, double c_K) -> int {
        magk::effective_values(pat, d_k, d_m, c_K, c_M, ctx->tr_aval.as<double>(), s);
        HIPCHK(hipGetLastError());
        return solver.system(ctx->tr_aval.as<double>());
    };
    // A_FF a = rhs_F from zero, a_P = 0, and the row's bookkeeping
    std::vector<int32_t> iterations(rows, 0);
    long long all_iterations = 0, most = 0;
    bool all_converged = true;
    auto solve = [&](int32_t row) -> int {
        if (int rc = solver.solve(d_rhs, ctx->tr_zero.as<double>(), st.a, nullptr, nullptr, "step %d", (int)row)) return rc;
        const mag_stats &cs = ctx->stats;
        iterations[(size_t)row] = (int32_t)cs.iterations;
        all_iterations += cs.iterations;
        most = std::max<long long>(most, cs.iterations);
        all_converged = all_converged && cs.converged != 0;
        return MAG_OK;
    };
    auto record_energies = [&](int64_t row) -> int {
        linear_energy_row(ctx, st, row, row);
        HIPCHK(hipGetLastError());
        return MAG_OK;
    };

    // ---- the start
    if (!resume) {
        magk::newmark_start(st, in.d_u0, in.d_v0, s);
        if (int rc = system(1.0, 0.0)) return rc;
        damped_rhs(ctx, st, st.u, st.v, alpha, eta, 0);
        if (int rc = solve(0)) return rc;
    }
    magk::newmark_record(st, 0, se > 0 ? d_snap : nullptr, s);
    if (energies)
        if (int rc = record_energies(0)) return rc;
    if (int rc = system(1.0 + gamma * dt * alpha, beta * dt * dt + gamma * dt * eta)) return rc;

    // ---- the steps
    for (int32_t n = 0; n < steps; ++n) {
        magk::newmark_predict(st, dt, beta, gamma, s);
        damped_rhs(ctx, st, st.ut, st.vt, alpha, eta, n + 1);
        if (int rc = solve(n + 1)) return rc;
        const bool snap = se > 0 && (n + 1) % se == 0;
        magk::newmark_correct(st, dt, beta, gamma, n + 1, snap ? d_snap + (size_t)((n + 1) / se) * (size_t)n2 : nullptr, s);
        if (energies)
            if (int rc = record_energies(n + 1)) return rc;
    }

    // ---- the reactions of the final state
    linear_reactions(ctx, st, alpha, eta, steps);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));

    int32_t *info = ctx->tr_info;
    info[0] = steps;
    info[1] = choice.fused ? 5 : 3;
    info[2] = choice.kind;
    info[3] = (int32_t)std::min<long long>(all_iterations, INT32_MAX);
    info[4] = (int32_t)most;
    info[5] = (int32_t)snaps;
    info[6] = resume ? 1 : 0;
    info[7] = all_converged ? 1 : 0;
    ctx->tr_iterations = iterations;
    publish_steps(ctx, so, energies, rows, snaps, t_start, dt, in.amp_last, 0.0, 0.0);
    if (!all_converged) ctx->err = std::string(fn) + ": a solve stopped at the iteration cap above the tolerance: its last iterate was used";
    return MAG_OK;
}

int mag_download_transient(mag_ctx *ctx, mag_transient_result *o)
{
    const char *fn = "mag_download_transient";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null result", fn);
    if (int rc = memory_refused(ctx, o->memory, fn)) return rc;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: transient dynamics run on one GPU: this context has a communicator of %d ranks", fn, ctx->comm.nranks);
    if (!ctx->have_problem || !ctx->tr_have) return fail(ctx, MAG_ERR_STATE, "%s before a completed mag_run_transient", fn);
    if (o->probe_u || o->probe_v || o->probe_a)
        if (ctx->tr_num_probes == 0) return fail(ctx, MAG_ERR_STATE, "%s: the run recorded no probes", fn);
    if (o->energies && !ctx->tr_energies) return fail(ctx, MAG_ERR_STATE, "%s: the run recorded no energies", fn);
    if (o->snapshots && ctx->tr_snaps == 0) return fail(ctx, MAG_ERR_STATE, "%s: the run kept no snapshots", fn);
    if (int rc = enter(ctx)) return rc;
    const auto [kind, hkind] = out_kinds(o->memory);
    hipStream_t s = ctx->stream;
    const size_t vb = 16 * (size_t)ctx->N, rows = (size_t)ctx->tr_rows, pb = 8 * rows * (size_t)ctx->tr_num_probes;
    if (o->u_out) HIPCHK(hipMemcpyAsync(o->u_out, ctx->tr_u.p, vb, kind, s));
    if (o->v_out) HIPCHK(hipMemcpyAsync(o->v_out, ctx->tr_v.p, vb, kind, s));
    if (o->a_out) HIPCHK(hipMemcpyAsync(o->a_out, ctx->tr_a.p, vb, kind, s));
    if (o->f_out) HIPCHK(hipMemcpyAsync(o->f_out, ctx->tr_f.p, vb, kind, s));
    if (o->probe_u) HIPCHK(hipMemcpyAsync(o->probe_u, ctx->tr_probe.p, pb, kind, s));
    if (o->probe_v) HIPCHK(hipMemcpyAsync(o->probe_v, ctx->tr_probe.as<char>() + pb, pb, kind, s));
    if (o->probe_a) HIPCHK(hipMemcpyAsync(o->probe_a, ctx->tr_probe.as<char>() + 2 * pb, pb, kind, s));
    if (o->energies) HIPCHK(hipMemcpyAsync(o->energies, ctx->tr_energy.p, 3 * 8 * rows, kind, s));
    if (o->snapshots) HIPCHK(hipMemcpyAsync(o->snapshots, ctx->tr_snap.p, (size_t)ctx->tr_snaps * vb, kind, s));
    if (o->iterations) HIPCHK(hipMemcpyAsync(o->iterations, ctx->tr_iterations.data(), 4 * rows, hkind, s));
    HIPCHK(hipStreamSynchronize(s));
    o->scalars[0] = ctx->tr_t0;
    o->scalars[1] = ctx->tr_t1;
    o->scalars[2] = ctx->tr_dt;
    o->scalars[3] = ctx->tr_dt_bound;
    return MAG_OK;
}

int mag_get_transient_info(const mag_ctx *ctx, int32_t info[8])
{
    if (!ctx || !info || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->have_problem || !ctx->tr_have) return MAG_ERR_STATE;
    for (int k = 0; k < 8; ++k) info[k] = ctx->tr_info[k];
    return MAG_OK;
}

// ---- explicit dynamics (explicit.hip): central differences on the lumped mass.  The driver shares the transient pass's
// matrices, records and result slots and the passes' table (ptab: the linear fused step's) and checks (chk_*); a step that
// records nothing is one launch, enqueued on the context's stream, and the host reads nothing between the launches ----
namespace {

// the stable step from lambda_bound: (2 / omega) (sqrt(1 + xi^2) - xi), xi = eta omega / 2, with the difference written as
// 1 / (sqrt(1 + xi^2) + xi) (no cancellation at a large xi)
double explicit_dt_bound(double lambda, double eta)
{
    const double omega = std::sqrt(lambda), xi = eta * omega / 2.0;
    return (2.0 / omega) / (std::sqrt(1.0 + xi * xi) + xi);
}

// out[0] lambda_bound, [1] dt_bound with eta = 0, [2] with eta, [3] the smallest node mass, of K and the lumped mass in place
// (transient_matrices); synchronises
int explicit_bounds(mag_ctx *ctx, double eta, double out[4])
{
    hipStream_t s = ctx->stream;
    HIPCHK(ctx->ex_part.reserve(8 * 2 * (size_t)magk::kSensBlocks));
    HIPCHK(ctx->ex_out.reserve(32));
    magk::explicit_bound(transient_pattern(ctx), ctx->kval.as<double>(), ctx->tr_mval.as<double>(), ctx->uknown.as<uint8_t>(),
                         ctx->ex_part.as<double>(), ctx->ex_out.as<double>(), s);
    HIPCHK(hipGetLastError());
    double h[2] = {0.0, 0.0};
    HIPCHK(hipMemcpyAsync(h, ctx->ex_out.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    out[0] = h[0];
    out[1] = explicit_dt_bound(h[0], 0.0);
    out[2] = explicit_dt_bound(h[0], eta);
    out[3] = h[1];
    return MAG_OK;
}

} // namespace

int mag_set_material_law(mag_ctx *ctx, int32_t law)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (law != MAG_LAW_SVK && law != MAG_LAW_NEO_HOOKE)
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_set_material_law: law = %d is neither MAG_LAW_SVK nor MAG_LAW_NEO_HOOKE", (int)law);
    ctx->law = law; // (read by the total-Lagrangian entry points alone: no stored result changes)
    return MAG_OK;
}

int mag_get_material_law(const mag_ctx *ctx, int32_t *law)
{
    if (!ctx || !law) return MAG_ERR_BAD_ARGS;
    *law = ctx->law;
    return MAG_OK;
}

void mag_default_explicit_options(mag_explicit_options *o)
{
    if (!o) return;
    *o = {};
    o->record_every = 1;
    o->dt_scale = 0.9;
}

int mag_explicit_dt(mag_ctx *ctx, double density, double rayleigh_stiffness, double out[4])
{
    const char *fn = "mag_explicit_dt";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!out) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null out", fn);
    if (int rc = need_pos(ctx, fn, {{"density", density}})) return rc;
    if (int rc = need_nonneg(ctx, fn, {{"rayleigh_stiffness", rayleigh_stiffness}})) return rc;
    if (int rc = transient_refused(ctx, fn)) return rc;
    if (int rc = enter(ctx)) return rc;
    if (int rc = transient_matrices(ctx, density, 1)) return rc;
    return explicit_bounds(ctx, rayleigh_stiffness, out);
}

int mag_run_explicit(mag_ctx *ctx, const mag_explicit_options *o)
{
    const char *fn = "mag_run_explicit";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null options", fn);
    if (o->steps < 1) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: steps = %d: at least one step", fn, (int)o->steps);
    if (int rc = need_nonneg(ctx, fn, {{"dt", o->dt}, {"dt_scale", o->dt_scale}})) return rc;
    if (int rc = need_pos(ctx, fn, {{"density", o->density}})) return rc;
    if (int rc = need_nonneg(ctx, fn, {{"rayleigh_mass", o->rayleigh_mass}, {"rayleigh_stiffness", o->rayleigh_stiffness}})) return rc;
    if (o->kinematics != MAG_KIN_LINEAR && o->kinematics != MAG_KIN_TOTAL_LAGRANGIAN)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: kinematics = %d is neither MAG_KIN_LINEAR nor MAG_KIN_TOTAL_LAGRANGIAN", fn, (int)o->kinematics);
    if (o->kinematics == MAG_KIN_TOTAL_LAGRANGIAN && o->rayleigh_stiffness != 0.0)
        return fail(ctx, MAG_ERR_BAD_ARGS,
                    "%s: rayleigh_stiffness %g must be 0 with kinematics = MAG_KIN_TOTAL_LAGRANGIAN (initial-stiffness damping is not objective)", fn,
                    o->rayleigh_stiffness);
    if (o->record_every < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: record_every = %d is negative", fn, (int)o->record_every);
    const StepOptions so = {o->steps, o->snapshot_every, o->num_probes, o->probes, o->memory, o->resume, o->amplitude, o->u0, o->v0};
    if (int rc = step_args_tail(ctx, fn, so)) return rc;
    if (o->kinematics == MAG_KIN_TOTAL_LAGRANGIAN)
        if (int rc = law_refused(ctx, fn)) return rc;

    const bool resume = o->resume != 0, energies = o->energies != 0, tl = o->kinematics == MAG_KIN_TOTAL_LAGRANGIAN;
    const int32_t steps = o->steps, np = o->num_probes, se = o->snapshot_every, re = o->record_every > 0 ? o->record_every : 1;
    const double alpha = o->rayleigh_mass, eta = o->rayleigh_stiffness;
    const double t_start = resume ? ctx->tr_t1 : 0.0;
    const double amp_first = ctx->tr_amp_last; // (a resumed run's row 0 carries the load of the state it resumes)
    ctx->tr_have = ctx->tt_have = false; // (a failure leaves no results of the pass)
    hipStream_t s = ctx->stream;

    if (int rc = transient_matrices(ctx, o->density, 1)) return rc;
    const bool fused = ctx->use_lds; // (known once the order is built: the tile-local tables, or a step of four launches)
    const int64_t N = ctx->N, n2 = 2 * N;
    const size_t vb = 16 * (size_t)N;
    const magk::Pattern pat = transient_pattern(ctx);

    // ---- the checks that need the device: the elements' orientation, the probes; the step
    StepWords words;
    if (int rc = step_checks_enqueue(ctx, so, &words)) return rc;
    double bounds[4];
    if (int rc = explicit_bounds(ctx, eta, bounds)) return rc; // (synchronises)
    if (int rc = step_checks_report(ctx, fn, words)) return rc;
    const double dt_bound = bounds[2];
    const double dt = o->dt != 0.0 ? o->dt : (o->dt_scale != 0.0 ? o->dt_scale : 0.9) * dt_bound;
    if (!pos_finite(dt)) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: dt = 0 asks for dt_scale * dt_bound, and dt_bound is %g (no free DOF carries stiffness)", fn, dt_bound);

    // ---- the buffers, the inputs
    const size_t rows = (size_t)(steps / re) + 1, amp_n = (size_t)steps + 1, snaps = se > 0 ? (size_t)(steps / se) + 1 : 0;
    if (int rc = step_buffers(ctx, fn, steps, rows, amp_n, snaps, np, resume)) return rc;
    StepInputs in;
    if (int rc = step_inputs(ctx, so, amp_n, amp_first, &in)) return rc;
    const magk::NewmarkState st = newmark_state(ctx, rows, np);
    magk::NewmarkState st_quiet = st; // (the state without the probes: a snapshot alone, the unfused step's corrector)
    st_quiet.num_probes = 0;
    double *d_rhs = ctx->tr_rhs.as<double>(), *d_energy = ctx->tr_energy.as<double>(), *d_snap = ctx->tr_snap.as<double>();
    double *d_amp = ctx->tr_amp.as<double>();
    const double *d_f = ctx->fin.as<double>(), *d_k = ctx->kval.as<double>(), *d_m = ctx->tr_mval.as<double>();
    StepWords *d_words = ctx->chk_words.as<StepWords>();

    // ---- total-Lagrangian kinematics (explicit_tl.hip): the mesh as the force kernel reads it, the inverted-element flag (the
    // probes' word is done with)
    const magk::TlMesh tlm = tl ? tl_mesh(ctx) : magk::TlMesh{};
    int32_t *d_inverted = &d_words->inverted;
    if (tl) HIPCHK(hipMemsetAsync(d_inverted, 0, 4, s));

    // ---- the fused step: the inputs and the records in Hilbert order and the frame of either kernel; the linear step's table and
    // values (unmasked: prescribed displacements enter through K ut) -- the total-Lagrangian step reads no matrix
    magk::ExplicitParams P = {};
    magk::ExplicitTlParams Q = {};
    magk::StepFrame &F = tl ? Q.f : P.f;
    int32_t grid = 1;
    int cur = 0;
    magk::ExRec *rec[2] = {nullptr, nullptr};
    if (fused && !tl) {
        FieldTable tab = pass_table(ctx);
        if (int rc = build_field_table(ctx, tab)) return rc;
        magk::field_gather(ctx->bptr.as<int32_t>(), ctx->perm.as<uint32_t>(), d_k, ctx->tr_zero.as<uint8_t>(), ctx->halo_g.as<int32_t>(),
                           tab.meta.as<magk::FieldTileMeta>(), tab.slot.as<uint16_t>(), tab.src.as<int32_t>(), N, ctx->B, ctx->T, tab.total,
                           tab.val.as<double2>(), s);
        P.total = tab.total;
        P.meta = tab.meta.as<magk::FieldTileMeta>(), P.slot = tab.slot.as<uint16_t>(), P.fval = tab.val.as<double2>();
        P.eta = eta;
    }
    if (fused) {
        for (DevBuf &b : ctx->ex_rec) HIPCHK(b.reserve(sizeof(magk::ExRec) * (size_t)N));
        HIPCHK(ctx->ex_mass.reserve(8 * (size_t)N));
        HIPCHK(ctx->ex_uin.reserve(vb));
        HIPCHK(ctx->ex_f.reserve(vb));
        magk::explicit_inputs(pat, ctx->perm.as<uint32_t>(), d_m, st.u_in, d_f, ctx->ex_mass.as<double>(), ctx->ex_uin.as<double2>(),
                              ctx->ex_f.as<double2>(), s);
        HIPCHK(hipGetLastError());
        rec[0] = ctx->ex_rec[0].as<magk::ExRec>();
        rec[1] = ctx->ex_rec[1].as<magk::ExRec>();
        F = step_frame(ctx, alpha);
    }
    if (fused && tl) {
        Q.xyP = ctx->xyP.as<double2>(), Q.halo_xy = ctx->halo_xy.as<double2>();
        Q.tile_deg = ctx->tile_rdeg.as<int32_t>(), Q.tile_off = ctx->tile_off.as<int64_t>(), Q.ell16 = ctx->ell.as<uint32_t>();
        Q.tile_hoff = ctx->tile_hoff.as<int32_t>();
        set_tl_material(ctx, Q);
        Q.inverted = d_inverted;
    }
    if (fused) grid = tl ? magk::explicit_tl_grid(ctx->B, ctx->cap, ctx->T, ctx->law) : magk::explicit_grid(ctx->B, ctx->cap, ctx->T);
    long long launches = 0;
    bool expanded = true; // (tr_u, tr_v, tr_a hold the current state)
    // one step of h (the start: h = 0) under amplitude[amp_at]
    auto step = [&](double h, int64_t amp_at) {
        if (fused) {
            F.in = rec[cur], F.out = rec[cur ^ 1], F.dt = h, F.amp_at = amp_at;
            if (tl)
                magk::explicit_tl_step(Q, ctx->B, grid, s);
            else
                magk::explicit_step(P, ctx->B, grid, s);
            cur ^= 1;
            expanded = false;
            launches += 1;
            return;
        }
        if (tl) {
            magk::newmark_predict(st, h, 0.0, 0.5, s);
            magk::tl_force(tlm, st.ut, d_rhs, d_inverted, nullptr, nullptr, s);
            magk::tl_divide(pat, d_m, st.known, d_f, d_amp, amp_at, d_rhs, st.vt, alpha, 1.0 + 0.5 * h * alpha, st.a, s);
            magk::newmark_correct(st_quiet, h, 0.0, 0.5, 0, nullptr, s);
            launches += 4;
            return;
        }
        magk::newmark_predict(st, h, 0.0, 0.5, s);
        damped_rhs(ctx, st, st.ut, st.vt, alpha, eta, amp_at);
        magk::explicit_divide(pat, d_m, st.known, d_rhs, 1.0 + 0.5 * h * alpha, st.a, s);
        magk::newmark_correct(st_quiet, h, 0.0, 0.5, 0, nullptr, s);
        launches += 4;
    };
    auto expand = [&]() {
        if (expanded) return;
        magk::explicit_scatter(ctx->perm.as<uint32_t>(), N, rec[cur], st.u, st.v, st.a, s);
        expanded = true;
    };
    // the records of step n: probe and energy row n / re when re divides n, the snapshot when se does
    auto record = [&](int32_t n) {
        // (a row without probes and energies holds nothing: such a step stays the one launch)
        const bool row_due = n % re == 0 && (np > 0 || energies), snap_due = se > 0 && n % se == 0;
        if (!row_due && !snap_due) return;
        expand();
        double *snap = snap_due ? d_snap + (size_t)(n / se) * (size_t)n2 : nullptr;
        const int64_t row = n / re;
        magk::newmark_record(row_due ? st : st_quiet, row, snap, s);
        if (row_due && energies && tl) {
            magk::tl_energies(tlm, pat, d_m, st.known, st.u, st.v, d_f, d_amp, n, d_inverted, ctx->tr_part.as<double>(), d_energy + 3 * row, s);
        } else if (row_due && energies) {
            linear_energy_row(ctx, st, row, n);
        }
    };

    // ---- the start: a_0 by the step with dt = 0
    if (!resume) magk::newmark_start(st, in.d_u0, in.d_v0, s);
    if (fused) magk::explicit_gather(ctx->perm.as<uint32_t>(), N, st.u, st.v, st.a, rec[cur], s);
    if (!resume) step(0.0, 0);
    record(0);
    HIPCHK(hipGetLastError());

    // ---- the steps
    for (int32_t n = 0; n < steps; ++n) {
        step(dt, n + 1);
        record(n + 1);
    }
    HIPCHK(hipGetLastError());

    // ---- the final state, its finite check and its reactions
    expand();
    int32_t *d_flag = &d_words->not_finite; // (the checks' words are done with)
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, s));
    magk::explicit_finite(st.u, st.v, st.a, n2, d_flag, s);
    if (tl) {
        magk::tl_force(tlm, st.u, d_rhs, d_inverted, nullptr, nullptr, s);
        magk::tl_reactions(st.known, d_f, d_amp, steps, d_rhs, n2, ctx->tr_f.as<double>(), s);
    } else {
        linear_reactions(ctx, st, alpha, eta, steps);
    }
    StepWords flags = {}; // (read back up to the inverted-element flag)
    HIPCHK(hipMemcpyAsync(&flags, d_words, tl ? offsetof(StepWords, inverted) + 4 : 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    const int32_t not_finite = flags.not_finite, inverted = tl ? flags.inverted : 0;
    if (not_finite)
        return fail(ctx, MAG_ERR_NOT_CONVERGED, "%s: the state after %d steps is not finite: dt = %g against dt_bound = %g (the step is unstable)", fn,
                    (int)steps, dt, dt_bound);

    int32_t *info = ctx->tr_info;
    info[0] = steps;
    info[1] = tl ? 7 : 6;
    info[2] = fused ? 1 : 0;
    info[3] = (int32_t)std::min<long long>(launches, INT32_MAX);
    info[4] = re;
    info[5] = (int32_t)snaps;
    info[6] = resume ? 1 : 0;
    info[7] = inverted ? 0 : 1;
    ctx->tr_iterations.assign(rows, 0);
    publish_steps(ctx, so, energies, rows, snaps, t_start, dt, in.amp_last, dt, dt_bound);
    return MAG_OK;
}

int mag_internal_force(mag_ctx *ctx, const double *u, double *f_out, double scalars_out[2], int32_t memory)
{
    const char *fn = "mag_internal_force";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!u) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null u", fn);
    if (!f_out) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null f_out", fn);
    if (!scalars_out) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null scalars_out", fn);
    if (int rc = memory_refused(ctx, memory, fn)) return rc;
    if (int rc = transient_refused(ctx, fn)) return rc;
    if (int rc = law_refused(ctx, fn)) return rc;
    if (int rc = enter(ctx)) return rc;
    if (int rc = ensure_order(ctx)) return rc;
    const size_t vb = 16 * (size_t)ctx->N;
    HIPCHK(ctx->tl_f.reserve(vb));
    HIPCHK(ctx->tl_part.reserve(8 * (size_t)magk::kSensBlocks));
    EvalWords h;
    auto force = [&](const double *d_u, EvalWords *d) {
        magk::tl_force(tl_mesh(ctx), d_u, ctx->tl_f.as<double>(), &d->inverted, ctx->tl_part.as<double>(), &d->W, ctx->stream);
    };
    if (int rc = evaluate_at(ctx, fn, u, memory, force, ctx->tl_f, vb, f_out, &h)) return rc;
    scalars_out[0] = h.W;
    scalars_out[1] = h.inverted ? 1.0 : 0.0;
    return MAG_OK;
}

// ---- nonlinear statics (newton.hip): Newton's method on the total-Lagrangian tangent, in load increments.  The driver owns the
// buffers and enqueues force, tangent, gather and solve of every iteration on the context's stream; between them the host reads
// one NewtonScalars record per evaluation and the CG's convergence polls, nothing else.  It shares the transient pass's solver
// (ImplicitSolver on ptab), device checks (step_checks_*, chk_*) and argument tail, and the loop's host logic (PhaseTimer,
// newton_stop, newton_unconverged) with mag_run_transient_tl; its state, records and results are its own (nt_*) ----
void mag_default_newton_options(mag_newton_options *o)
{
    if (!o) return;
    *o = {};
    o->increments = 1;
}

int mag_assemble_tangent(mag_ctx *ctx, const double *u, double *values_out, int32_t memory)
{
    const char *fn = "mag_assemble_tangent";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!u) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null u", fn);
    if (!values_out) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null values_out", fn);
    if (int rc = memory_refused(ctx, memory, fn)) return rc;
    if (int rc = transient_refused(ctx, fn)) return rc;
    if (int rc = law_refused(ctx, fn)) return rc;
    if (int rc = enter(ctx)) return rc;
    if (int rc = ensure_csr(ctx)) return rc;
    const size_t ab = 32 * (size_t)ctx->nb;
    HIPCHK(ctx->nt_kval.reserve(ab));
    EvalWords h;
    auto tangent = [&](const double *d_u, EvalWords *d) {
        magk::tl_tangent(tl_mesh(ctx), transient_pattern(ctx), d_u, ctx->nt_kval.as<double>(), &d->inverted, ctx->stream);
    };
    return evaluate_at(ctx, fn, u, memory, tangent, ctx->nt_kval, ab, values_out, &h);
}

int mag_run_newton(mag_ctx *ctx, const mag_newton_options *o)
{
    using magk::NewtonScalars;
    const char *fn = "mag_run_newton";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null options", fn);
    if (o->increments < 1) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: increments = %d: at least one increment", fn, (int)o->increments);
    if (o->max_newton < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: max_newton = %d is negative", fn, (int)o->max_newton);
    if (o->line_search < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: line_search = %d is negative", fn, (int)o->line_search);
    if (int rc = need_nonneg(ctx, fn, {{"newton_tol", o->newton_tol}, {"cg_tol", o->cg_tol}})) return rc;
    if (o->cg < 0 || o->cg > 4) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: cg = %d outside 0..4", fn, (int)o->cg);
    const StepOptions so = {o->increments, 0, o->num_probes, o->probes, o->memory, 0, nullptr, o->u0, nullptr};
    if (int rc = step_args_tail(ctx, fn, so)) return rc;
    if (int rc = law_refused(ctx, fn)) return rc;

    const int32_t incs = o->increments, np = o->num_probes, H = o->line_search;
    const int32_t cap = o->max_newton > 0 ? o->max_newton : 25;
    const double tol = o->newton_tol != 0.0 ? o->newton_tol : 1e-10, cg_tol = o->cg_tol != 0.0 ? o->cg_tol : 1e-10;
    const bool snapshots = o->snapshots != 0;
    ctx->nt_have = false; // (a failure leaves no results of the pass)
    hipStream_t s = ctx->stream;
    const hipMemcpyKind in_kind = in_kind_of(so.memory);

    if (int rc = ensure_csr(ctx)) return rc;
    if (int rc = reserve_cg(ctx)) return rc;
    const int64_t N = ctx->N, n2 = 2 * N;
    const size_t vb = 16 * (size_t)N, rows = (size_t)incs + 1;
    const magk::Pattern pat = transient_pattern(ctx);
    const magk::TlMesh mesh = tl_mesh(ctx);

    // ---- the checks that need the device: the elements' orientation, the probes
    StepWords words;
    if (int rc = step_checks_enqueue(ctx, so, &words)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = step_checks_report(ctx, fn, words)) return rc;

    ImplicitSolver::Choice choice;
    if (int rc = ImplicitSolver::choose(ctx, fn, o->cg, &choice)) return rc;

    // ---- the buffers, the inputs
    for (DevBuf *b : {&ctx->nt_u, &ctx->nt_ut, &ctx->nt_uc, &ctx->nt_du, &ctx->nt_dup, &ctx->nt_zero, &ctx->nt_f, &ctx->nt_rhs, &ctx->nt_fout})
        HIPCHK(b->reserve(vb));
    HIPCHK(ctx->nt_kval.reserve(32 * (size_t)ctx->nb));
    HIPCHK(ctx->nt_elem.reserve(64 * (size_t)ctx->E));
    HIPCHK(ctx->nt_load.reserve(8 * rows));
    HIPCHK(ctx->nt_probe.reserve(8 * rows * (size_t)std::max(np, 1)));
    HIPCHK(ctx->nt_snap.reserve(snapshots ? rows * vb : 8));
    HIPCHK(ctx->nt_part.reserve(8 * 5 * (size_t)magk::kSensBlocks));
    HIPCHK(ctx->nt_scal.reserve(sizeof(NewtonScalars) + 8)); // (behind the record: the flag of the element rows)
    HIPCHK(hipMemsetAsync(ctx->nt_zero.p, 0, vb, s));
    HIPCHK(hipMemsetAsync(ctx->nt_probe.p, 0, 8 * rows * (size_t)std::max(np, 1), s));
    if (snapshots) HIPCHK(hipMemsetAsync(ctx->nt_snap.p, 0, rows * vb, s));
    std::vector<double> loads(rows, 0.0);
    double *d_load = ctx->nt_load.as<double>();
    if (o->load_factors) {
        HIPCHK(hipMemsetAsync(d_load, 0, 8, s));
        HIPCHK(hipMemcpyAsync(d_load + 1, o->load_factors, 8 * (size_t)incs, in_kind, s));
        HIPCHK(hipMemcpyAsync(loads.data(), d_load, 8 * rows, hipMemcpyDeviceToHost, s));
    } else {
        for (int32_t k = 1; k <= incs; ++k) loads[(size_t)k] = (double)k / (double)incs;
        HIPCHK(hipMemcpyAsync(d_load, loads.data(), 8 * rows, hipMemcpyHostToDevice, s));
    }
    if (o->u0)
        HIPCHK(hipMemcpyAsync(ctx->nt_u.p, o->u0, vb, in_kind, s));
    else
        HIPCHK(hipMemsetAsync(ctx->nt_u.p, 0, vb, s));
    HIPCHK(hipStreamSynchronize(s)); // (the host's copies are done with)

    double *d_u = ctx->nt_u.as<double>(), *d_ut = ctx->nt_ut.as<double>(), *d_uc = ctx->nt_uc.as<double>();
    double *d_du = ctx->nt_du.as<double>(), *d_dup = ctx->nt_dup.as<double>(), *d_f = ctx->nt_f.as<double>(), *d_rhs = ctx->nt_rhs.as<double>();
    double *d_kt = ctx->nt_kval.as<double>(), *d_snap = ctx->nt_snap.as<double>(), *d_part = ctx->nt_part.as<double>();
    const double *d_zero = ctx->nt_zero.as<double>(), *d_fin = ctx->fin.as<double>(), *d_uin = ctx->uin.as<double>();
    const uint8_t *d_known = ctx->uknown.as<uint8_t>();
    const int32_t *d_probes = ctx->chk_probes.as<int32_t>();
    NewtonScalars *d_scal = ctx->nt_scal.as<NewtonScalars>();

    ImplicitSolver solver(ctx, fn, choice, cg_tol);
    if (int rc = solver.init()) return rc;
    // K_T,FF du_F = rhs_F from zero, du_P = dP (the support part of the step, or zero), on the solver's copy of the tangent in nt_kval
    std::vector<int32_t> newton_its(rows, 0), cg_its;
    std::vector<double> energies(2 * rows, 0.0), residuals, steps;
    long long all_cg = 0, halvings = 0;
    auto solve = [&](int32_t inc, int32_t it, const double *dP) -> int {
        if (int rc = solver.solve(d_rhs, dP, d_du, nullptr, nullptr, "increment %d, iteration %d", (int)inc, (int)it)) return rc;
        cg_its.push_back((int32_t)solver.prev);
        all_cg += solver.prev;
        return MAG_OK;
    };
    // f_int, W and the norms of the state w under load[at] (with du: the slope too, of the force that is in nt_f already)
    auto evaluate = [&](const double *w, int64_t at, NewtonScalars *h) -> int {
        HIPCHK(hipMemsetAsync(&d_scal->inverted, 0, 4, s));
        magk::tl_force(mesh, w, d_f, &d_scal->inverted, d_part, &d_scal->W, s);
        magk::newton_norms(d_known, d_fin, d_load, at, d_f, w, nullptr, n2, d_part, d_scal, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h, d_scal, sizeof(NewtonScalars), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return MAG_OK;
    };
    auto record = [&](int64_t row, const NewtonScalars &h) {
        magk::newton_record(d_uc, d_probes, np, row, ctx->nt_probe.as<double>(), snapshots ? d_snap + (size_t)row * (size_t)n2 : nullptr, n2, s);
        energies[2 * (size_t)row] = h.W;
        energies[2 * (size_t)row + 1] = h.W - loads[(size_t)row] * h.fu;
    };

    // the phases of every iteration: tangent + right-hand side, gather, CG, update + force + norms
    PhaseTimer timer(ctx, "MAG_TUNE_NEWTON_TIMES", 4);

    // ---- the start
    NewtonScalars cur = {};
    if (int rc = evaluate(d_u, 0, &cur)) return rc;
    HIPCHK(hipMemcpyAsync(d_uc, d_u, vb, hipMemcpyDeviceToDevice, s));
    record(0, cur);
    bool inverted = false;
    int32_t done = 0;
    std::string unconverged;

    // ---- the increments
    for (int32_t k = 1; k <= incs; ++k) {
        const double lam = loads[(size_t)k];
        bool converged = false;
        bool first = true; // the supports are not at lam u_in yet: until an iteration with s = 1 has moved them
        double ratio = 0.0;
        for (int32_t it = 1; it <= cap && !converged; ++it) {
            if (int rc = timer.stamp(0)) return rc;
            magk::tl_tangent(mesh, pat, d_u, d_kt, &d_scal->inverted, s);
            magk::newton_rhs(pat, d_kt, d_known, d_fin, d_load, k, d_f, d_u, d_uin, first ? 1 : 0, d_rhs, d_dup, s);
            HIPCHK(hipGetLastError());
            if (int rc = timer.stamp(1)) return rc;
            if (int rc = solver.system(d_kt)) return rc;
            if (int rc = timer.stamp(2)) return rc;
            if (int rc = solve(k, it, first ? d_dup : d_zero)) return rc;
            if (int rc = timer.stamp(3)) return rc;
            double slope = 0.0;
            const double Pi0 = cur.W - lam * cur.fu;
            if (H > 0) { // the slope of Pi along the step, of the force still in nt_f
                NewtonScalars hs = {};
                magk::newton_norms(d_known, d_fin, d_load, k, d_f, d_u, d_du, n2, d_part, d_scal, s);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(&hs, d_scal, sizeof(NewtonScalars), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                slope = hs.slope;
            }
            double sl = 1.0;
            NewtonScalars trial = {};
            for (int32_t hv = 0;; ++hv) {
                magk::newton_update(d_u, d_du, sl, n2, d_ut, s);
                if (int rc = evaluate(d_ut, k, &trial)) return rc;
                const double Pi_t = trial.W - lam * trial.fu;
                const bool energy = slope < 0.0 && std::fabs(sl * slope) > 1e-13 * std::max(std::fabs(Pi0), cur.W) && Pi_t > Pi0 + 1e-4 * sl * slope;
                if (hv == H || !(trial.inverted || energy)) break;
                sl *= 0.5;
                ++halvings;
            }
            if (int rc = timer.stamp(4)) return rc;
            if (int rc = timer.add(true)) return rc;
            std::swap(d_u, d_ut);
            cur = trial;
            inverted = inverted || cur.inverted != 0;
            first = first && sl != 1.0; // (a shortened step leaves them short: the next iteration predicts the rest)
            const NewtonStop stop = newton_stop(cur.r2, std::max(cur.f2, cur.p2), tol);
            ratio = stop.ratio, converged = stop.converged && !first;
            residuals.push_back(ratio);
            steps.push_back(sl);
            if (converged) newton_its[(size_t)k] = it;
        }
        if (!converged) {
            newton_unconverged(unconverged, fn, "increment", k, cap, ratio, cap, tol);
            break;
        }
        HIPCHK(hipMemcpyAsync(d_uc, d_u, vb, hipMemcpyDeviceToDevice, s));
        record(k, cur);
        done = k;
    }
    for (size_t k = (size_t)done + 1; k < rows; ++k) loads[k] = 0.0;

    // ---- the results of the last converged state: its reactions, its element rows
    int32_t *d_flag = (int32_t *)(d_scal + 1);
    magk::tl_force(mesh, d_uc, d_f, d_flag, d_part, nullptr, s);
    magk::tl_reactions(d_known, d_fin, d_load, done, d_f, n2, ctx->nt_fout.as<double>(), s);
    magk::newton_elements(mesh, d_uc, tl_stress_scale(ctx), ctx->nt_elem.as<double>(), d_flag, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));

    int32_t *info = ctx->nt_info;
    info[0] = done;
    info[1] = choice.fused ? 5 : 3;
    info[2] = choice.kind;
    info[3] = (int32_t)residuals.size();
    info[4] = (int32_t)std::min<long long>(all_cg, INT32_MAX);
    info[5] = (int32_t)std::min<long long>(halvings, INT32_MAX);
    info[6] = inverted ? 1 : 0;
    info[7] = done == incs ? 1 : 0;
    ctx->nt_increments = incs;
    ctx->nt_num_probes = np;
    ctx->nt_snaps = snapshots ? (int32_t)rows : 0;
    ctx->nt_loads = loads;
    ctx->nt_energies = energies;
    ctx->nt_residuals = residuals;
    ctx->nt_steps = steps;
    ctx->nt_newton = newton_its;
    ctx->nt_cg = cg_its;
    ctx->nt_have = true;
    timer.append("{\"newton_iterations\": %d, \"cg_iterations\": %lld, \"tangent_ms\": %.6f, \"gather_ms\": %.6f, \"cg_ms\": %.6f, \"force_ms\": %.6f}\n",
                 (int)residuals.size(), all_cg, timer.ms[0], timer.ms[1], timer.ms[2], timer.ms[3]);
    if (!unconverged.empty()) ctx->err = unconverged;
    return MAG_OK;
}

int mag_download_newton(mag_ctx *ctx, mag_newton_result *o)
{
    const char *fn = "mag_download_newton";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null result", fn);
    if (int rc = memory_refused(ctx, o->memory, fn)) return rc;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: transient dynamics run on one GPU: this context has a communicator of %d ranks", fn, ctx->comm.nranks);
    if (!ctx->have_problem || !ctx->nt_have) return fail(ctx, MAG_ERR_STATE, "%s before a completed mag_run_newton", fn);
    if (o->probe_u && ctx->nt_num_probes == 0) return fail(ctx, MAG_ERR_STATE, "%s: the run recorded no probes", fn);
    if (o->snapshots && ctx->nt_snaps == 0) return fail(ctx, MAG_ERR_STATE, "%s: the run kept no snapshots", fn);
    if (int rc = enter(ctx)) return rc;
    const auto [kind, hkind] = out_kinds(o->memory);
    hipStream_t s = ctx->stream;
    const size_t vb = 16 * (size_t)ctx->N, rows = (size_t)ctx->nt_increments + 1, its = ctx->nt_residuals.size();
    if (o->u_out) HIPCHK(hipMemcpyAsync(o->u_out, ctx->nt_uc.p, vb, kind, s));
    if (o->f_out) HIPCHK(hipMemcpyAsync(o->f_out, ctx->nt_fout.p, vb, kind, s));
    if (o->elem) HIPCHK(hipMemcpyAsync(o->elem, ctx->nt_elem.p, 64 * (size_t)ctx->E, kind, s));
    if (o->probe_u) HIPCHK(hipMemcpyAsync(o->probe_u, ctx->nt_probe.p, 8 * rows * (size_t)ctx->nt_num_probes, kind, s));
    if (o->snapshots) HIPCHK(hipMemcpyAsync(o->snapshots, ctx->nt_snap.p, rows * vb, kind, s));
    if (o->load) HIPCHK(hipMemcpyAsync(o->load, ctx->nt_loads.data(), 8 * rows, hkind, s));
    if (o->energies) HIPCHK(hipMemcpyAsync(o->energies, ctx->nt_energies.data(), 16 * rows, hkind, s));
    if (o->newton_iterations) HIPCHK(hipMemcpyAsync(o->newton_iterations, ctx->nt_newton.data(), 4 * rows, hkind, s));
    if (its > 0) {
        if (o->residuals) HIPCHK(hipMemcpyAsync(o->residuals, ctx->nt_residuals.data(), 8 * its, hkind, s));
        if (o->cg_iterations) HIPCHK(hipMemcpyAsync(o->cg_iterations, ctx->nt_cg.data(), 4 * its, hkind, s));
        if (o->step_lengths) HIPCHK(hipMemcpyAsync(o->step_lengths, ctx->nt_steps.data(), 8 * its, hkind, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int mag_get_newton_info(const mag_ctx *ctx, int32_t info[8])
{
    if (!ctx || !info || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->have_problem || !ctx->nt_have) return MAG_ERR_STATE;
    for (int k = 0; k < 8; ++k) info[k] = ctx->nt_info[k];
    return MAG_OK;
}

// ---- nonlinear transient dynamics (transient_tl.hip): Newmark's method on the total-Lagrangian internal force, every step by
// Newton's method on the effective tangent.  The driver owns its matrix and work buffers (tt_*), shares the step frame of
// mag_run_transient / mag_run_explicit (the checks, the inputs, the records, the result slots), their solver (ImplicitSolver on
// ptab) and the Newton loop's host logic of mag_run_newton; between the launches the host reads one TlStepScalars record per Newton
// iteration and the CG's convergence polls, nothing else ----
void mag_default_transient_tl_options(mag_transient_tl_options *o)
{
    if (!o) return;
    *o = {};
    o->beta = 0.25;
    o->gamma = 0.5;
}

int mag_assemble_effective_tangent(mag_ctx *ctx, const double *u, double c_K, double c_M, double density, int32_t lumped, double *values_out,
                                   int32_t memory)
{
    const char *fn = "mag_assemble_effective_tangent";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!u) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null u", fn);
    if (!values_out) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null values_out", fn);
    if (!std::isfinite(c_K) || !std::isfinite(c_M)) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: c_K %g / c_M %g is not finite", fn, c_K, c_M);
    if (int rc = need_pos(ctx, fn, {{"density", density}})) return rc;
    if (int rc = memory_refused(ctx, memory, fn)) return rc;
    if (int rc = transient_refused(ctx, fn)) return rc;
    if (int rc = law_refused(ctx, fn)) return rc;
    if (int rc = enter(ctx)) return rc;
    if (int rc = transient_matrices(ctx, density, lumped)) return rc;
    const size_t ab = 32 * (size_t)ctx->nb;
    HIPCHK(ctx->tt_aval.reserve(ab));
    EvalWords h;
    auto tangent = [&](const double *d_u, EvalWords *d) {
        magk::tl_effective_tangent(tl_mesh(ctx), transient_pattern(ctx), d_u, ctx->tr_mval.as<double>(), c_K, c_M, ctx->tt_aval.as<double>(),
                                   &d->inverted, ctx->stream);
    };
    return evaluate_at(ctx, fn, u, memory, tangent, ctx->tt_aval, ab, values_out, &h);
}

int mag_run_transient_tl(mag_ctx *ctx, const mag_transient_tl_options *o)
{
    using magk::TlStepScalars;
    const char *fn = "mag_run_transient_tl";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null options", fn);
    if (o->steps < 1) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: steps = %d: at least one step", fn, (int)o->steps);
    if (int rc = need_pos(ctx, fn, {{"dt", o->dt}, {"density", o->density}})) return rc;
    if (int rc = need_nonneg(ctx, fn, {{"beta", o->beta}})) return rc;
    if (o->beta == 0.0)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: beta = 0 leaves no system to solve: the explicit step is mag_run_explicit's (kinematics = MAG_KIN_TOTAL_LAGRANGIAN)",
                    fn);
    if (int rc = need_nonneg(ctx, fn, {{"gamma", o->gamma}, {"rayleigh_mass", o->rayleigh_mass}, {"cg_tol", o->cg_tol}, {"newton_tol", o->newton_tol}}))
        return rc;
    if (o->max_newton < 0) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: max_newton = %d is negative", fn, (int)o->max_newton);
    if (o->cg < 0 || o->cg > 4) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: cg = %d outside 0..4", fn, (int)o->cg);
    const StepOptions so = {o->steps, o->snapshot_every, o->num_probes, o->probes, o->memory, o->resume, o->amplitude, o->u0, o->v0};
    if (int rc = step_args_tail(ctx, fn, so)) return rc;
    if (int rc = law_refused(ctx, fn)) return rc;

    const bool resume = o->resume != 0, energies = o->energies != 0;
    const int32_t steps = o->steps, np = o->num_probes, se = o->snapshot_every;
    const int32_t cap = o->max_newton > 0 ? o->max_newton : 25;
    const double dt = o->dt, beta = o->beta, gamma = o->gamma, alpha = o->rayleigh_mass;
    const double tol = o->newton_tol != 0.0 ? o->newton_tol : 1e-10, cg_tol = o->cg_tol != 0.0 ? o->cg_tol : 1e-10;
    const double c_u = beta * dt * dt, c_v = gamma * dt, c_M = 1.0 + gamma * dt * alpha;
    const double t_start = resume ? ctx->tr_t1 : 0.0;
    const double amp_first = ctx->tr_amp_last; // (a resumed run's row 0 carries the load of the state it resumes)
    ctx->tr_have = ctx->tt_have = false; // (a failure leaves no results of the pass)
    hipStream_t s = ctx->stream;

    if (int rc = transient_matrices(ctx, o->density, o->lumped)) return rc;
    if (int rc = reserve_cg(ctx)) return rc;
    const int64_t N = ctx->N, n2 = 2 * N;
    const size_t vb = 16 * (size_t)N;
    const magk::Pattern pat = transient_pattern(ctx);
    const magk::TlMesh mesh = tl_mesh(ctx);

    // ---- the checks that need the device: the elements' orientation, the probes
    StepWords words;
    if (int rc = step_checks_enqueue(ctx, so, &words)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = step_checks_report(ctx, fn, words)) return rc;

    ImplicitSolver::Choice choice;
    if (int rc = ImplicitSolver::choose(ctx, fn, o->cg, &choice)) return rc;

    // ---- the buffers, the inputs
    const size_t rows = (size_t)steps + 1, snaps = se > 0 ? (size_t)(steps / se) + 1 : 0;
    if (int rc = step_buffers(ctx, fn, steps, rows, rows, snaps, np, resume)) return rc;
    StepInputs in;
    if (int rc = step_inputs(ctx, so, rows, amp_first, &in)) return rc;
    const magk::NewmarkState st = newmark_state(ctx, rows, np);
    for (DevBuf *b : {&ctx->tt_an, &ctx->tt_un, &ctx->tt_vn, &ctx->tt_da, &ctx->tt_fint}) HIPCHK(b->reserve(vb));
    HIPCHK(ctx->tt_aval.reserve(32 * (size_t)ctx->nb));
    HIPCHK(ctx->tt_elem.reserve(64 * (size_t)ctx->E));
    HIPCHK(ctx->tt_part.reserve(8 * 4 * (size_t)magk::kSensBlocks));
    HIPCHK(ctx->tt_scal.reserve(sizeof(TlStepScalars) + 8)); // (behind the record: the flag of the element rows)
    double *d_rhs = ctx->tr_rhs.as<double>(), *d_snap = ctx->tr_snap.as<double>(), *d_amp = ctx->tr_amp.as<double>();
    double *d_an = ctx->tt_an.as<double>(), *d_un = ctx->tt_un.as<double>(), *d_vn = ctx->tt_vn.as<double>(), *d_da = ctx->tt_da.as<double>();
    double *d_fint = ctx->tt_fint.as<double>(), *d_at = ctx->tt_aval.as<double>(), *d_part = ctx->tt_part.as<double>();
    const double *d_m = ctx->tr_mval.as<double>(), *d_f = ctx->fin.as<double>(), *d_zero = ctx->tr_zero.as<double>();
    TlStepScalars *d_scal = ctx->tt_scal.as<TlStepScalars>();
    HIPCHK(hipMemsetAsync(d_scal, 0, sizeof(TlStepScalars) + 8, s));

    ImplicitSolver solver(ctx, fn, choice, cg_tol);
    if (int rc = solver.init()) return rc;
    // A_T = cm M + ck K_T(w) in tt_aval, one launch
    auto tangent = [&](double cm, double ck, const double *w) -> int {
        magk::tl_effective_tangent(mesh, pat, w, d_m, ck, cm, d_at, &d_scal->inverted, s);
        HIPCHK(hipGetLastError());
        return MAG_OK;
    };
    // the phases of every iteration: tangent; gather; into the solver's numbering; CG; back + state + force + residual
    PhaseTimer timer(ctx, "MAG_TUNE_TRANSIENT_TL_TIMES", 5);
    // A_T,FF x_F = rhs_F from zero, x_P = 0: the transient pass's poll scheme
    std::vector<int32_t> iterations(rows, 0), newton_its(rows, 0), cg_its;
    std::vector<double> residuals;
    long long all_cg = 0;
    auto solve = [&](int32_t step, int32_t it, double *x) -> int {
        if (int rc = solver.solve(d_rhs, d_zero, x, timer.event(3), timer.event(4), "step %d, iteration %d", (int)step, (int)it)) return rc;
        iterations[(size_t)step] = (int32_t)std::min<long long>((long long)iterations[(size_t)step] + solver.prev, INT32_MAX);
        all_cg += solver.prev;
        return MAG_OK;
    };
    // f_int(w) and the residual of (w, av, vv) under amplitude[at] into tr_rhs, its norms into the record
    auto residual = [&](const double *w, const double *av, const double *vv, int64_t at) -> int {
        magk::tl_force(mesh, w, d_fint, &d_scal->inverted, nullptr, nullptr, s);
        magk::tl_residual(pat, d_m, st.known, d_f, d_amp, at, d_fint, av, vv, alpha, d_rhs, d_part, d_scal, s);
        HIPCHK(hipGetLastError());
        return MAG_OK;
    };
    auto record_energies = [&](int64_t row) -> int {
        magk::tl_dynamic_energies(mesh, pat, d_m, st.known, st.u, st.v, d_f, d_amp, row, &d_scal->inverted, ctx->tr_part.as<double>(),
                                  ctx->tr_energy.as<double>() + 3 * row, s);
        HIPCHK(hipGetLastError());
        return MAG_OK;
    };

    // ---- the start: M_FF a_0 = (amp[0] f - alpha M v_0 - f_int(u_0))_F.  The matrix is M alone, by the linear pass's
    // effective_values on K with (c_M, c_K) = (1, 0): no tangent is evaluated for a factor of zero
    if (!resume) {
        magk::newmark_start(st, in.d_u0, in.d_v0, s);
        if (int rc = residual(st.u, d_zero, st.v, 0)) return rc;
        magk::effective_values(pat, ctx->kval.as<double>(), d_m, 0.0, 1.0, d_at, s);
        HIPCHK(hipGetLastError());
        if (int rc = solver.system(d_at)) return rc;
        if (int rc = solve(0, 0, st.a)) return rc;
    }
    magk::newmark_record(st, 0, se > 0 ? d_snap : nullptr, s);
    if (energies)
        if (int rc = record_energies(0)) return rc;

    // ---- the steps
    magk::TlTrial trial = {n2, st.known, st.u, st.ut, st.vt, d_an, d_da, d_an, d_un, d_vn};
    int32_t done = 0, most = 0;
    bool inverted = false;
    std::string unconverged;
    for (int32_t n = 0; n < steps; ++n) {
        magk::newmark_predict(st, dt, beta, gamma, s);
        magk::tl_trial_state(trial, 1.0, c_u, c_v, 1, s); // the first iterate: u' = u_n
        if (int rc = residual(d_un, d_an, d_vn, n + 1)) return rc;
        bool converged = false;
        double ratio = 0.0;
        int32_t it = 0;
        while (it < cap && !converged) {
            ++it;
            if (int rc = timer.stamp(0)) return rc;
            if (int rc = tangent(c_M, c_u, d_un)) return rc;
            if (int rc = timer.stamp(1)) return rc;
            if (int rc = solver.system(d_at)) return rc;
            if (int rc = timer.stamp(2)) return rc;
            if (int rc = solve(n + 1, it, d_da)) return rc; // (records events 3 and 4 around the CG)
            magk::tl_trial_state(trial, 1.0, c_u, c_v, 0, s);
            if (int rc = residual(d_un, d_an, d_vn, n + 1)) return rc;
            TlStepScalars h = {};
            HIPCHK(hipMemcpyAsync(&h, d_scal, sizeof(TlStepScalars), hipMemcpyDeviceToHost, s));
            if (int rc = timer.stamp(5)) return rc;
            HIPCHK(hipStreamSynchronize(s));
            if (int rc = timer.add(false)) return rc;
            inverted = inverted || h.inverted != 0;
            const NewtonStop stop = newton_stop(h.r2, std::max(h.f2, std::max(h.i2, h.m2)), tol);
            ratio = stop.ratio, converged = stop.converged;
            residuals.push_back(ratio);
            cg_its.push_back((int32_t)solver.prev);
        }
        most = std::max(most, it);
        if (!converged) {
            newton_unconverged(unconverged, fn, "step", n + 1, cap, ratio, it, tol);
            break;
        }
        newton_its[(size_t)n + 1] = it;
        HIPCHK(hipMemcpyAsync(st.u, d_un, vb, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(st.v, d_vn, vb, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(st.a, d_an, vb, hipMemcpyDeviceToDevice, s));
        const bool snap = se > 0 && (n + 1) % se == 0;
        magk::newmark_record(st, n + 1, snap ? d_snap + (size_t)((n + 1) / se) * (size_t)n2 : nullptr, s);
        if (energies)
            if (int rc = record_energies(n + 1)) return rc;
        done = n + 1;
    }

    // ---- a run that ended early keeps the rows of its converged steps: the probes' three blocks move together (through a buffer of
    // the pass's: the blocks may overlap), the last amplitude is the last converged step's
    const size_t rows_done = (size_t)done + 1;
    double amp_last = in.amp_last;
    if (done < steps) {
        iterations.resize(rows_done);
        newton_its.resize(rows_done);
        HIPCHK(hipMemcpyAsync(&amp_last, d_amp + done, 8, hipMemcpyDeviceToHost, s));
        if (np > 0) {
            const size_t blk = 8 * rows_done * (size_t)np;
            HIPCHK(ctx->tt_move.reserve(blk));
            for (size_t b = 1; b < 3; ++b) {
                HIPCHK(hipMemcpyAsync(ctx->tt_move.p, st.probe_u + b * rows * (size_t)np, blk, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpyAsync(st.probe_u + b * rows_done * (size_t)np, ctx->tt_move.p, blk, hipMemcpyDeviceToDevice, s));
            }
        }
    }

    // ---- the results of the last converged state: its reactions, its element rows
    int32_t *d_flag = (int32_t *)(d_scal + 1);
    magk::tl_force(mesh, st.u, d_fint, d_flag, nullptr, nullptr, s);
    magk::tl_dynamic_reactions(pat, d_m, st.known, d_f, d_amp, done, d_fint, st.a, st.v, alpha, ctx->tr_f.as<double>(), s);
    magk::newton_elements(mesh, st.u, tl_stress_scale(ctx), ctx->tt_elem.as<double>(), d_flag, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));

    const size_t snaps_done = se > 0 ? (size_t)(done / se) + 1 : 0;
    long long step_most = 0, step_all = 0;
    for (int32_t v : iterations) step_most = std::max<long long>(step_most, v), step_all += v;
    int32_t *info = ctx->tr_info;
    info[0] = done;
    info[1] = choice.fused ? 5 : 3;
    info[2] = choice.kind;
    info[3] = (int32_t)std::min<long long>(step_all, INT32_MAX);
    info[4] = (int32_t)step_most;
    info[5] = (int32_t)snaps_done;
    info[6] = resume ? 1 : 0;
    info[7] = done == steps ? 1 : 0;
    int32_t *ti = ctx->tt_info;
    ti[0] = done;
    ti[1] = choice.fused ? 5 : 3;
    ti[2] = choice.kind;
    ti[3] = (int32_t)residuals.size();
    ti[4] = most;
    ti[5] = (int32_t)std::min<long long>(all_cg, INT32_MAX);
    ti[6] = inverted ? 1 : 0;
    ti[7] = done == steps ? 1 : 0;
    ctx->tr_iterations = iterations;
    ctx->tt_newton = newton_its;
    ctx->tt_cg = cg_its;
    ctx->tt_residuals = residuals;
    StepOptions published = so;
    published.steps = done;
    publish_steps(ctx, published, energies, rows_done, snaps_done, t_start, dt, amp_last, 0.0, 0.0);
    ctx->tt_have = true;
    timer.append("{\"steps\": %d, \"newton_iterations\": %d, \"cg_iterations\": %lld, \"tangent_ms\": %.6f, \"gather_ms\": %.6f, \"cg_ms\": %.6f, \"state_ms\": %.6f}\n",
                 (int)done, (int)residuals.size(), all_cg, timer.ms[0], timer.ms[1], timer.ms[3], timer.ms[2] + timer.ms[4]);
    if (!unconverged.empty()) ctx->err = unconverged;
    return MAG_OK;
}

int mag_download_transient_tl(mag_ctx *ctx, mag_transient_tl_result *o)
{
    const char *fn = "mag_download_transient_tl";
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "%s: null result", fn);
    if (int rc = memory_refused(ctx, o->memory, fn)) return rc;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "%s: transient dynamics run on one GPU: this context has a communicator of %d ranks", fn, ctx->comm.nranks);
    if (!ctx->have_problem || !ctx->tr_have || !ctx->tt_have) return fail(ctx, MAG_ERR_STATE, "%s before a completed mag_run_transient_tl", fn);
    if (int rc = enter(ctx)) return rc;
    const auto [kind, hkind] = out_kinds(o->memory);
    hipStream_t s = ctx->stream;
    const size_t its = ctx->tt_residuals.size();
    if (o->newton_iterations) HIPCHK(hipMemcpyAsync(o->newton_iterations, ctx->tt_newton.data(), 4 * ctx->tt_newton.size(), hkind, s));
    if (its > 0) {
        if (o->cg_iterations) HIPCHK(hipMemcpyAsync(o->cg_iterations, ctx->tt_cg.data(), 4 * its, hkind, s));
        if (o->residuals) HIPCHK(hipMemcpyAsync(o->residuals, ctx->tt_residuals.data(), 8 * its, hkind, s));
    }
    if (o->elem) HIPCHK(hipMemcpyAsync(o->elem, ctx->tt_elem.p, 64 * (size_t)ctx->E, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int mag_get_transient_tl_info(const mag_ctx *ctx, int32_t info[8])
{
    if (!ctx || !info || ctx->comm.nranks > 1) return MAG_ERR_BAD_ARGS;
    if (!ctx->have_problem || !ctx->tr_have || !ctx->tt_have) return MAG_ERR_STATE;
    for (int k = 0; k < 8; ++k) info[k] = ctx->tt_info[k];
    return MAG_OK;
}

// ---- mesh refinement (refine.hip): longest-edge bisection with conformity closure of the uploaded mesh.  The driver owns the
// buffers, runs the sorts and scans between the kernels' stages and reads back three times: the indicator's check (rules 1, 2),
// the sweeps' "changed" words once per batch, the sizes N' and E' to allocate ----
namespace {

// the checks mag_get_refine_info, mag_download_refine and mag_upload_refined share, before any HIP call
int refined_refused(const mag_ctx *ctx, const void *o, const char *what, const char *fn)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    mag_ctx *c = const_cast<mag_ctx *>(ctx); // (the message only)
    if (!o) return fail(c, MAG_ERR_BAD_ARGS, "%s: null %s", fn, what);
    if (!ctx->have_problem || !ctx->rf_have) return fail(c, MAG_ERR_STATE, "%s before a completed mag_run_refine", fn);
    return MAG_OK;
}

} // namespace

int mag_run_refine(mag_ctx *ctx, const mag_refine_options *ro)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (ctx->field_on) return field_refuses(ctx, "mag_run_refine");
    if (!ro) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_refine: null options");
    const int32_t rule = ro->rule, split = ro->split;
    if (rule < MAG_REFINE_MARKS || rule > MAG_REFINE_TOP_FRACTION)
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_refine: rule %d is none of enum mag_refine_rule", (int)rule);
    if (split != 1 && split != 3) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_refine: split = %d is neither 1 nor 3", (int)split);
    const bool by_indicator = rule != MAG_REFINE_MARKS;
    if (by_indicator && !(std::isfinite(ro->theta) && ro->theta > 0.0 && ro->theta <= 1.0))
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_refine: theta = %g outside (0, 1]", ro->theta);
    if (!by_indicator && !ro->marks) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_refine: null marks under MAG_REFINE_MARKS");
    if (!by_indicator || ro->indicator) // (the array the rule reads; a NULL indicator is the device's own eta2)
        if (int rc = memory_refused(ctx, ro->memory, "mag_run_refine")) return rc;
    if (ctx->comm.nranks > 1)
        return fail(ctx, MAG_ERR_BAD_ARGS, "refinement runs on one GPU: this context has a communicator of %d ranks", ctx->comm.nranks);
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "mag_run_refine before mag_upload");
    const DerivedSet &recovery = ctx->derived[PASS_STRESS][MAG_SET_RUN];
    if (by_indicator && !ro->indicator && !(ctx->have_run && recovery.have))
        return fail(ctx, MAG_ERR_STATE, "mag_run_refine: no indicator given and none held: before a completed mag_run_stress(MAG_SET_RUN)");
    if (int rc = enter(ctx)) return rc;

    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N, E = ctx->E;
    const size_t n3 = 3 * (size_t)E;
    ctx->rf_have = false;

    // the tables: one allocation, every part on a 256-byte boundary
    magk::RefineTables t = {};
    size_t bytes = 0;
    const auto part = [&bytes](size_t b) {
        const size_t at = bytes;
        bytes += (b + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_key0 = part(8 * n3), o_key1 = part(8 * n3), o_val0 = part(4 * n3), o_val1 = part(4 * n3), o_head = part(4 * n3),
                 o_hscan = part(4 * n3), o_eid = part(4 * n3), o_ekey = part(8 * n3), o_flag = part(4 * (n3 + 1)),
                 o_mid = part(4 * (n3 + 1)), o_lng = part((size_t)E), o_marks = part((size_t)E), o_cnt = part(4 * ((size_t)E + 1)),
                 o_off = part(4 * ((size_t)E + 1)), o_counters = part(4 * magk::RF_COUNTERS), o_check = part(16);
    HIPCHK(ctx->rf_tab.reserve(bytes));
    char *base = ctx->rf_tab.as<char>();
    t.N = N;
    t.E = E;
    t.xy = ctx->xy.as<double>();
    t.conn = ctx->conn.as<int32_t>();
    t.u_known = ctx->uknown.as<uint8_t>();
    t.u_in = ctx->uin.as<double>();
    t.f_in = ctx->fin.as<double>();
    t.key0 = (uint64_t *)(base + o_key0);
    t.key1 = (uint64_t *)(base + o_key1);
    t.val0 = (uint32_t *)(base + o_val0);
    t.val1 = (uint32_t *)(base + o_val1);
    t.head = (int32_t *)(base + o_head);
    t.hscan = (int32_t *)(base + o_hscan);
    t.eid = (int32_t *)(base + o_eid);
    t.ekey = (uint64_t *)(base + o_ekey);
    t.flag = (uint32_t *)(base + o_flag);
    t.mid = (int32_t *)(base + o_mid);
    t.lng = (uint8_t *)(base + o_lng);
    t.marks = (uint8_t *)(base + o_marks);
    t.cnt = (int32_t *)(base + o_cnt);
    t.off = (int32_t *)(base + o_off);
    t.counters = (uint32_t *)(base + o_counters);
    t.check = (uint64_t *)(base + o_check);

    // (the sorts and scans with a temporary of the pass's own)
    const auto sort64 = [&](const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, size_t n, int end_bit) -> int {
        size_t tb = 0;
        HIPCHK(magp::sort_pairs_u64(nullptr, &tb, kin, kout, vin, vout, n, 0, end_bit, s));
        HIPCHK(ctx->rf_tmp.reserve(tb));
        HIPCHK(magp::sort_pairs_u64(ctx->rf_tmp.p, &tb, kin, kout, vin, vout, n, 0, end_bit, s));
        return MAG_OK;
    };
    const auto scan32 = [&](const int32_t *in, int32_t *out, size_t n) -> int {
        size_t tb = 0;
        HIPCHK(magp::exclusive_scan_i32(nullptr, &tb, in, out, n, s));
        HIPCHK(ctx->rf_tmp.reserve(tb));
        HIPCHK(magp::exclusive_scan_i32(ctx->rf_tmp.p, &tb, in, out, n, s));
        return MAG_OK;
    };

    // 1. edges: keys, sort, run heads, ids, the longest edge of every element
    HIPCHK(hipMemsetAsync(t.flag, 0, 4 * (n3 + 1), s));
    HIPCHK(hipMemsetAsync(t.counters, 0, 4 * magk::RF_COUNTERS, s));
    magk::refine_edge_keys(t, s);
    if (int rc = sort64(t.key0, t.key1, t.val0, t.val1, n3, 32 + ceil_log2(N))) return rc;
    magk::refine_heads(t, s);
    if (int rc = scan32(t.head, t.hscan, n3)) return rc;
    magk::refine_edge_table(t, s);
    HIPCHK(hipGetLastError());

    // 2. marked elements
    const hipMemcpyKind kind = ro->memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!by_indicator) {
        HIPCHK(hipMemcpyAsync(t.marks, ro->marks, (size_t)E, kind, s));
    } else {
        const double *ind = recovery.seta2.as<double>(); // (member 0 of MAG_SET_RUN's recovery, where it lies)
        if (ro->indicator) {
            ind = ro->indicator;
            if (ro->memory != MAG_MEM_DEVICE) {
                HIPCHK(ctx->rf_in.reserve(8 * (size_t)E));
                HIPCHK(hipMemcpyAsync(ctx->rf_in.p, ro->indicator, 8 * (size_t)E, hipMemcpyHostToDevice, s));
                ind = ctx->rf_in.as<double>();
            }
        }
        const uint64_t check0[2] = {0, ~uint64_t(0)};
        uint64_t check[2] = {};
        HIPCHK(hipMemcpyAsync(t.check, check0, sizeof check0, hipMemcpyHostToDevice, s));
        magk::refine_check_indicator(t, ind, s);
        HIPCHK(hipMemcpyAsync(check, t.check, sizeof check, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (check[1] != ~uint64_t(0)) {
            double bad = 0.0;
            HIPCHK(hipMemcpy(&bad, ind + check[1], 8, hipMemcpyDeviceToHost));
            return fail(ctx, MAG_ERR_BAD_ARGS, "mag_run_refine: indicator[%lld] = %g is not finite and >= 0", (long long)check[1], bad);
        }
        if (rule == MAG_REFINE_MAX_FRACTION) {
            double vmax;
            memcpy(&vmax, &check[0], 8);
            if (vmax > 0.0) {
                const double threshold = ro->theta * vmax; // rounded once
                magk::refine_mark_max(t, ind, threshold, s);
            } else {
                HIPCHK(hipMemsetAsync(t.marks, 0, (size_t)E, s));
            }
        } else {
            const int64_t k = std::min<int64_t>(std::max<int64_t>((int64_t)std::ceil(ro->theta * (double)E), 1), E);
            HIPCHK(hipMemsetAsync(t.marks, 0, (size_t)E, s));
            magk::refine_top_keys(t, ind, s);
            if (int rc = sort64(t.key0, t.key1, t.val0, t.val1, (size_t)E, 64)) return rc;
            magk::refine_mark_top(t, k, s);
        }
    }
    magk::refine_mark_edges(t, split, s);
    HIPCHK(hipGetLastError());

    // 3. closure: batches of sweeps, their "changed" words read back once per batch; at most E + 1 sweeps
    int64_t sweeps = 0;
    for (bool done = false; !done;) {
        const int batch = (int)std::min<int64_t>(magk::kRefineSweepBatch, E + 1 - sweeps);
        if (batch < 1) return fail(ctx, MAG_ERR_STATE, "mag_run_refine: the closure did not end within %lld sweeps", (long long)(E + 1));
        uint32_t changed[magk::kRefineSweepBatch] = {};
        HIPCHK(hipMemsetAsync(t.counters + magk::RF_CHANGED, 0, sizeof changed, s));
        magk::refine_sweeps(t, batch, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(changed, t.counters + magk::RF_CHANGED, sizeof changed, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int j = 0; j < batch && !done; ++j) {
            ++sweeps;
            done = changed[j] == 0;
        }
    }

    // 4. counts, numbering, sizes
    magk::refine_child_counts(t, s);
    if (int rc = scan32((const int32_t *)t.flag, t.mid, n3 + 1)) return rc;
    if (int rc = scan32(t.cnt, t.off, (size_t)E + 1)) return rc;
    magk::refine_sizes(t, s);
    HIPCHK(hipGetLastError());
    uint32_t counters[magk::RF_COUNTERS] = {};
    HIPCHK(hipMemcpyAsync(counters, t.counters, sizeof counters, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int64_t Nn = N + (int64_t)counters[magk::RF_NEW_NODES], En = (int64_t)counters[magk::RF_NEW_ELEMS];
    if (Nn >= (int64_t(1) << 30) || 9 * En >= (int64_t(1) << 31))
        return fail(ctx, MAG_ERR_TOO_LARGE, "refined mesh too large for int32 indexing (nodes=%lld elements=%lld)", (long long)Nn, (long long)En);

    // 5. the refined mesh: the old nodes verbatim, the new nodes, the elements
    HIPCHK(ctx->rf_xy.reserve(16 * (size_t)Nn));
    HIPCHK(ctx->rf_conn.reserve(12 * (size_t)En));
    HIPCHK(ctx->rf_uknown.reserve(2 * (size_t)Nn));
    HIPCHK(ctx->rf_uin.reserve(16 * (size_t)Nn));
    HIPCHK(ctx->rf_fin.reserve(16 * (size_t)Nn));
    HIPCHK(ctx->rf_nparents.reserve(8 * (size_t)(Nn - N)));
    HIPCHK(ctx->rf_eparent.reserve(4 * (size_t)En));
    HIPCHK(hipMemcpyAsync(ctx->rf_xy.p, ctx->xy.p, 16 * (size_t)N, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->rf_uknown.p, ctx->uknown.p, 2 * (size_t)N, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->rf_uin.p, ctx->uin.p, 16 * (size_t)N, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->rf_fin.p, ctx->fin.p, 16 * (size_t)N, hipMemcpyDeviceToDevice, s));
    magk::RefinedMesh out = {ctx->rf_xy.as<double>(), ctx->rf_conn.as<int32_t>(), ctx->rf_uknown.as<uint8_t>(), ctx->rf_uin.as<double>(),
                             ctx->rf_fin.as<double>(), ctx->rf_nparents.as<int32_t>(), ctx->rf_eparent.as<int32_t>()};
    magk::refine_emit(t, out, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    const int64_t info[8] = {Nn, En, (int64_t)counters[magk::RF_MARKED], Nn - N, sweeps, (int64_t)counters[magk::RF_SPLIT2],
                             (int64_t)counters[magk::RF_SPLIT3], (int64_t)counters[magk::RF_SPLIT4]};
    memcpy(ctx->rf_info, info, sizeof info);
    ctx->rf_have = true;
    return MAG_OK;
}

int mag_get_refine_info(const mag_ctx *ctx, int64_t info[8])
{
    if (int rc = refined_refused(ctx, info, "info", "mag_get_refine_info")) return rc;
    memcpy(info, ctx->rf_info, sizeof ctx->rf_info);
    return MAG_OK;
}

int mag_download_refine(mag_ctx *ctx, mag_refined *o)
{
    if (ctx && o)
        if (int rc = memory_refused(ctx, o->memory, "mag_download_refine")) return rc;
    if (int rc = refined_refused(ctx, o, "refined mesh", "mag_download_refine")) return rc;
    if (int rc = enter(ctx)) return rc;
    const hipMemcpyKind kind = o->memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipStream_t s = ctx->stream;
    const size_t Nn = (size_t)ctx->rf_info[0], En = (size_t)ctx->rf_info[1], added = (size_t)ctx->rf_info[3];
    if (o->xy) HIPCHK(hipMemcpyAsync(o->xy, ctx->rf_xy.p, 16 * Nn, kind, s));
    if (o->conn) HIPCHK(hipMemcpyAsync(o->conn, ctx->rf_conn.p, 12 * En, kind, s));
    if (o->u_known) HIPCHK(hipMemcpyAsync(o->u_known, ctx->rf_uknown.p, 2 * Nn, kind, s));
    if (o->u_in) HIPCHK(hipMemcpyAsync(o->u_in, ctx->rf_uin.p, 16 * Nn, kind, s));
    if (o->f_in) HIPCHK(hipMemcpyAsync(o->f_in, ctx->rf_fin.p, 16 * Nn, kind, s));
    if (o->node_parents && added) HIPCHK(hipMemcpyAsync(o->node_parents, ctx->rf_nparents.p, 8 * added, kind, s));
    if (o->elem_parent) HIPCHK(hipMemcpyAsync(o->elem_parent, ctx->rf_eparent.p, 4 * En, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

// The refined mesh through mag_upload itself, its arrays read where they lie: what mag_upload does to the context is done, and
// only the refinement's arrays, which it drops, are held again
int mag_upload_refined(mag_ctx *ctx)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!ctx->have_problem || !ctx->rf_have) return fail(ctx, MAG_ERR_STATE, "mag_upload_refined before a completed mag_run_refine");
    mag_problem p = {};
    p.num_nodes = ctx->rf_info[0];
    p.num_elements = ctx->rf_info[1];
    p.xy = ctx->rf_xy.as<double>();
    p.conn = ctx->rf_conn.as<int32_t>();
    p.u_known = ctx->rf_uknown.as<uint8_t>();
    p.u_in = ctx->rf_uin.as<double>();
    p.f_in = ctx->rf_fin.as<double>();
    p.youngs_modulus = ctx->youngs;
    p.poisson_ratio = ctx->nu;
    p.part_thickness = ctx->thick;
    p.memory = MAG_MEM_DEVICE;
    if (int rc = mag_upload(ctx, &p)) return rc;
    ctx->rf_have = true;
    return MAG_OK;
}

// ---- the element stiffness field and the density design update on it ----
namespace {

// A new field (or none) is in place: the single run's and the load cases' results and what was derived from them go; the order,
// the tables and the pattern stay when the context already ran under a field (they were built with the CSR operator's choices)
void field_installed(mag_ctx *ctx, bool on)
{
    if (on != ctx->field_on) ctx->have_order = ctx->field_sym = false;
    ctx->field_on = on;
    ctx->have_csr = ctx->have_run = false;
    ctx->cases.have_run = false;
    for (int32_t slot = MAG_SET_RUN; slot <= MAG_SET_CASES; ++slot) {
        drop_derived(ctx, slot);
        ctx->adj[slot].have = ctx->adj[slot].have_run = false;
    }
}

// the first entry of x[0 .. n) that is not finite, <= 0 or > upper: -1 when there is none
int first_bad_entry(mag_ctx *ctx, const double *x, int64_t n, double upper, int32_t &first)
{
    hipStream_t s = ctx->stream;
    HIPCHK(ctx->ds_small.reserve(8 * magk::DW_COUNT + 16));
    int32_t *flag = (int32_t *)(ctx->ds_small.as<double>() + magk::DW_COUNT);
    first = INT32_MAX;
    HIPCHK(hipMemcpyAsync(flag, &first, 4, hipMemcpyHostToDevice, s));
    magk::first_out_of_range(x, n, upper, flag, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&first, flag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (first == INT32_MAX) first = -1;
    return MAG_OK;
}

magk::DesignParams design_params(const mag_ctx *ctx)
{
    const mag_design_options &o = ctx->design_opt;
    return {o.scale_min, o.rho_min, o.move, o.volume_fraction, o.penal, o.filter_passes};
}

// out = F^passes x (forward) or (F^T)^passes x; out may not be x; ds_tmp: two rows of E, ds_node: N
int design_filter_passes(mag_ctx *ctx, const magk::SensMesh &mesh, bool transpose, const double *x, double *out)
{
    hipStream_t s = ctx->stream;
    const size_t eb = 8 * (size_t)ctx->E;
    const int32_t P = ctx->design_opt.filter_passes;
    if (P == 0) {
        HIPCHK(hipMemcpyAsync(out, x, eb, hipMemcpyDeviceToDevice, s));
        return MAG_OK;
    }
    double *tmp[2] = {ctx->ds_tmp.as<double>(), ctx->ds_tmp.as<double>() + ctx->E};
    const double *cur = x;
    for (int32_t k = 0; k < P; ++k) {
        double *nxt = k == P - 1 ? out : tmp[k & 1];
        if (transpose)
            magk::design_filter_t(mesh, ctx->xy.as<double>(), ctx->ds_area.as<double>(), ctx->ds_node_area.as<double>(), cur,
                                  ctx->ds_node.as<double>(), nxt, s);
        else
            magk::design_filter(mesh, ctx->xy.as<double>(), ctx->ds_area.as<double>(), ctx->ds_node_area.as<double>(), cur,
                                ctx->ds_node.as<double>(), nxt, s);
        cur = nxt;
    }
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

// rho~ = F^P rho, s = scale_min + (1 - scale_min) rho~^p into the context's field, the greyness word
int design_interpolate_field(mag_ctx *ctx, const magk::SensMesh &mesh)
{
    hipStream_t s = ctx->stream;
    if (int rc = design_filter_passes(ctx, mesh, false, ctx->ds_rho.as<double>(), ctx->ds_rhof.as<double>())) return rc;
    magk::design_interpolate(ctx->ds_rhof.as<double>(), ctx->E, design_params(ctx), ctx->escale.as<double>(), s);
    magk::design_greyness(ctx->ds_rhof.as<double>(), ctx->E, ctx->ds_part.as<double>(), ctx->ds_small.as<double>(), s);
    HIPCHK(hipGetLastError());
    return MAG_OK;
}

int design_read_info(mag_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(ctx->design_info, ctx->ds_small.as<double>() + magk::DW_INFO, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

} // namespace

int mag_set_element_scale(mag_ctx *ctx, const double *scale, int32_t memory)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (scale && !memory_known(memory)) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_set_element_scale: memory = %d is none of enum mag_memory", (int)memory);
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "mag_set_element_scale before mag_upload");
    if (scale)
        if (int rc = field_context_refused(ctx, "mag_set_element_scale")) return rc;
    if (int rc = enter(ctx)) return rc;
    if (!scale) { // clear: the context computes what it computed before the field
        ctx->design_on = false;
        if (ctx->field_on) field_installed(ctx, false);
        return MAG_OK;
    }
    hipStream_t s = ctx->stream;
    const int64_t E = ctx->E;
    HIPCHK(ctx->ds_tmp.reserve(2 * 8 * (size_t)E));
    HIPCHK(hipMemcpyAsync(ctx->ds_tmp.p, scale, 8 * (size_t)E, memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    int32_t bad = -1;
    if (int rc = first_bad_entry(ctx, ctx->ds_tmp.as<double>(), E, HUGE_VAL, bad)) return rc;
    if (bad >= 0)
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_set_element_scale: scale[%d] is not finite and > 0 (the field is as it was)", (int)bad);
    HIPCHK(ctx->escale.reserve(8 * (size_t)E));
    HIPCHK(hipMemcpyAsync(ctx->escale.p, ctx->ds_tmp.p, 8 * (size_t)E, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    ctx->design_on = false; // (a field of the caller's ends a design)
    field_installed(ctx, true);
    return MAG_OK;
}

int mag_design_init(mag_ctx *ctx, const mag_design_options *o, const double *rho0, int32_t memory)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: null options");
    const auto inside = [](double v, bool closed_above) { return std::isfinite(v) && v > 0.0 && (closed_above ? v <= 1.0 : v < 1.0); };
    if (!inside(o->volume_fraction, true))
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: volume_fraction = %g outside (0, 1]", o->volume_fraction);
    if (!inside(o->scale_min, false)) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: scale_min = %g outside (0, 1)", o->scale_min);
    if (!inside(o->rho_min, false)) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: rho_min = %g outside (0, 1)", o->rho_min);
    if (!inside(o->move, true)) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: move = %g outside (0, 1]", o->move);
    if (o->penal < 1 || o->penal > 8) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: penal = %d outside 1..8", (int)o->penal);
    if (o->filter_passes < 0 || o->filter_passes > 8)
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: filter_passes = %d outside 0..8", (int)o->filter_passes);
    if (rho0 && !memory_known(memory)) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: memory = %d is none of enum mag_memory", (int)memory);
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "mag_design_init before mag_upload");
    if (int rc = field_context_refused(ctx, "mag_design_init")) return rc;
    if (int rc = enter(ctx)) return rc;
    hipStream_t s = ctx->stream;
    const int64_t N = ctx->N, E = ctx->E;
    const size_t eb = 8 * (size_t)E;
    ctx->design_on = false;
    ctx->design_opt = *o;
    // The filter walks the incidence lists: the order and the tables are built here, with the CSR operator's choices as every
    // context under a field has them.  The design's scale becomes the context's field at the END, once everything is checked:
    // a refused init leaves a field of the caller's, and the results under it, as they were (a design in progress is ended).
    struct Undo { // ... and an order built here does not outlive a refused init on a context without a field
        mag_ctx *ctx;
        bool armed;
        ~Undo()
        {
            if (armed) ctx->have_order = false;
        }
    } undo{ctx, !ctx->field_on};
    if (!ctx->field_on) ctx->have_order = false;
    {
        FieldOperator op(ctx, true);
        if (int rc = ensure_order(ctx)) return rc;
    }
    magk::SensMesh mesh;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    if (int rc = reserve_rows(ctx, {ROWS(ctx->ds_rho, eb), ROWS(ctx->ds_rhof, eb), ROWS(ctx->ds_w, eb), ROWS(ctx->ds_area, eb),
                                    ROWS(ctx->ds_tmp, 2 * eb), ROWS(ctx->ds_dJ, eb), ROWS(ctx->ds_dJdrho, eb), ROWS(ctx->ds_bq, eb),
                                    ROWS(ctx->ds_rho_new, eb), ROWS(ctx->escale, eb), ROWS(ctx->ds_node_area, 8 * (size_t)N),
                                    ROWS(ctx->ds_node, 8 * (size_t)N), ROWS(ctx->ds_part, 8 * magk::kDesignPartials),
                                    ROWS(ctx->ds_small, 8 * magk::DW_COUNT + 16)}, 1))
        return rc;
    double *small = ctx->ds_small.as<double>(), *part = ctx->ds_part.as<double>();
    int32_t *flag = (int32_t *)(small + magk::DW_COUNT);
    HIPCHK(hipMemsetAsync(small, 0, 8 * magk::DW_COUNT, s));
    HIPCHK(hipMemsetAsync(ctx->ds_dJdrho.p, 0, eb, s));
    int32_t bad = INT32_MAX;
    HIPCHK(hipMemcpyAsync(flag, &bad, 4, hipMemcpyHostToDevice, s));
    magk::design_areas(mesh, ctx->xy.as<double>(), ctx->ds_area.as<double>(), flag, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad != INT32_MAX)
        return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: element %d has a signed area <= 0 (counter-clockwise elements are required)", (int)bad);
    if (rho0) {
        HIPCHK(hipMemcpyAsync(ctx->ds_rho.p, rho0, eb, memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        if (int rc = first_bad_entry(ctx, ctx->ds_rho.as<double>(), E, 1.0, bad)) return rc;
        if (bad >= 0) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_init: rho0[%d] is outside (0, 1]", (int)bad);
    } else {
        const std::vector<double> uniform((size_t)E, o->volume_fraction);
        HIPCHK(hipMemcpyAsync(ctx->ds_rho.p, uniform.data(), eb, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    magk::design_node_areas(mesh, ctx->xy.as<double>(), ctx->ds_area.as<double>(), ctx->ds_node_area.as<double>(), s);
    magk::design_total_area(ctx->ds_area.as<double>(), E, o->volume_fraction, part, small, s);
    HIPCHK(hipGetLastError());
    // w = (F^T)^P a: the filtered volume is sum_e w_e rho_e exactly, no filter inside the bisection
    if (int rc = design_filter_passes(ctx, mesh, true, ctx->ds_area.as<double>(), ctx->ds_w.as<double>())) return rc;
    magk::design_volume(ctx->ds_rho.as<double>(), ctx->ds_w.as<double>(), E, part, small, s);
    if (int rc = design_interpolate_field(ctx, mesh)) return rc;
    if (int rc = design_read_info(ctx)) return rc;
    undo.armed = false;
    const bool order_kept = ctx->have_order;
    field_installed(ctx, true);
    ctx->have_order = order_kept; // (built above under the field's choices)
    ctx->design_steps = 0;
    ctx->design_on = true;
    return MAG_OK;
}

int mag_design_step(mag_ctx *ctx, const double *dJ_ds, int32_t memory)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (dJ_ds && !memory_known(memory)) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_design_step: memory = %d is none of enum mag_memory", (int)memory);
    if (!ctx->design_on) return fail(ctx, MAG_ERR_STATE, "mag_design_step before mag_design_init");
    if (!ctx->have_run) return fail(ctx, MAG_ERR_STATE, "mag_design_step before a completed mag_run under the design's scale");
    const DerivedSet &sens = ctx->derived[PASS_SENS][MAG_SET_RUN];
    if (!dJ_ds && !sens.have)
        return fail(ctx, MAG_ERR_STATE, "mag_design_step with a NULL gradient before mag_run_sensitivities(MAG_SET_RUN) of this run");
    if (int rc = enter(ctx)) return rc;
    hipStream_t s = ctx->stream;
    const int64_t E = ctx->E;
    const size_t eb = 8 * (size_t)E;
    const magk::DesignParams dp = design_params(ctx);
    magk::SensMesh mesh;
    if (int rc = sens_mesh(ctx, mesh)) return rc;
    const double J = dJ_ds ? 0.0 : -2.0 * sens.scalars_h[1];
    const double *given = nullptr;
    if (dJ_ds) {
        given = ctx->ds_dJ.as<double>();
        HIPCHK(hipMemcpyAsync(ctx->ds_dJ.p, dJ_ds, eb, memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    }
    // dJ/drho~ (into ds_bq, free until the update), then dJ/drho = (F^T)^P of it
    magk::design_chain(given, sens.energy.as<double>(), ctx->escale.as<double>(), ctx->ds_rhof.as<double>(), E, dp, ctx->ds_bq.as<double>(), s);
    if (int rc = design_filter_passes(ctx, mesh, true, ctx->ds_bq.as<double>(), ctx->ds_dJdrho.as<double>())) return rc;
    magk::design_oc(ctx->ds_rho.as<double>(), ctx->ds_dJdrho.as<double>(), ctx->ds_w.as<double>(), E, dp, ctx->ds_bq.as<double>(),
                    ctx->ds_rho_new.as<double>(), ctx->ds_part.as<double>(), ctx->ds_small.as<double>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctx->ds_rho.p, ctx->ds_rho_new.p, eb, hipMemcpyDeviceToDevice, s));
    if (int rc = design_interpolate_field(ctx, mesh)) return rc;
    if (int rc = design_read_info(ctx)) return rc;
    ctx->design_info[5] = (double)++ctx->design_steps;
    ctx->design_info[6] = J;
    ctx->design_info[7] = 0.0;
    field_installed(ctx, true); // the new scale: the run it was derived from is gone
    return MAG_OK;
}

int mag_get_design_info(const mag_ctx *ctx, double info[8])
{
    if (!ctx || !info) return MAG_ERR_BAD_ARGS;
    if (!ctx->design_on) return MAG_ERR_STATE;
    for (int k = 0; k < 8; ++k) info[k] = ctx->design_info[k];
    return MAG_OK;
}

int mag_download_design(mag_ctx *ctx, const mag_design *o)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    if (!o) return fail(ctx, MAG_ERR_BAD_ARGS, "null design");
    if (!memory_known(o->memory)) return fail(ctx, MAG_ERR_BAD_ARGS, "mag_download_design: memory = %d is none of enum mag_memory", (int)o->memory);
    if (!ctx->design_on) return fail(ctx, MAG_ERR_STATE, "mag_download_design before mag_design_init");
    if (int rc = enter(ctx)) return rc;
    const hipMemcpyKind kind = o->memory == MAG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipStream_t s = ctx->stream;
    const size_t eb = 8 * (size_t)ctx->E;
    if (o->rho_out) HIPCHK(hipMemcpyAsync(o->rho_out, ctx->ds_rho.p, eb, kind, s));
    if (o->rho_filtered_out) HIPCHK(hipMemcpyAsync(o->rho_filtered_out, ctx->ds_rhof.p, eb, kind, s));
    if (o->scale_out) HIPCHK(hipMemcpyAsync(o->scale_out, ctx->escale.p, eb, kind, s));
    if (o->dJ_drho_out) HIPCHK(hipMemcpyAsync(o->dJ_drho_out, ctx->ds_dJdrho.p, eb, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int mag_solve(mag_ctx *ctx, const mag_problem *p, mag_result *r)
{
    if (ctx && p) // (both structs before the upload: a refused result leaves the context as it was)
        if (int rc = memory_refused(ctx, p->memory, "mag_solve")) return rc;
    if (ctx && r)
        if (int rc = memory_refused(ctx, r->memory, "mag_solve")) return rc;
    if (int rc = mag_upload(ctx, p)) return rc;
    const int rc_run = mag_run(ctx);
    if (rc_run != MAG_OK && rc_run != MAG_ERR_NOT_CONVERGED) return rc_run; // a breakdown still hands back what it has
    if (r) {
        const std::string keep = ctx->err;
        if (int rc = mag_download(ctx, r)) return rc;
        ctx->err = keep;
    }
    return rc_run;
}

int mag_get_stats(const mag_ctx *ctx, mag_stats *st)
{
    if (!ctx || !st) return MAG_ERR_BAD_ARGS;
    *st = ctx->stats;
    return MAG_OK;
}

int mag_get_history(mag_ctx *ctx, double *history, int64_t n)
{
    if (int rc = enter(ctx)) return rc;
    if (!ctx->have_run && !ctx->cases.have_run && !ctx->variants.have_run) return fail(ctx, MAG_ERR_STATE, "no completed run");
    if (n < 0 || n > ctx->opt.history_len || n > ctx->stats.iterations || (n > 0 && !history))
        return fail(ctx, MAG_ERR_BAD_ARGS, "history length %lld not available", (long long)n);
    if (n > 0) HIPCHK(hipMemcpy(history, ctx->hist.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
    return MAG_OK;
}

int mag_element_stiffness(mag_ctx *ctx, double *ke_out)
{
    if (int rc = enter(ctx)) return rc;
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "no problem uploaded");
    if (!ke_out) return fail(ctx, MAG_ERR_BAD_ARGS, "null output");
    if (int rc = ensure_order(ctx)) return rc; // validates conn before it is dereferenced
    if (int rc = element_phase(ctx)) return rc;
    HIPCHK(hipMemcpyAsync(ke_out, ctx->ke.p, 8 * 36 * (size_t)ctx->E, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MAG_OK;
}

int mag_assemble_csr(mag_ctx *ctx, int64_t *nnz, int32_t *rowptr, int32_t *col, double *val)
{
    if (int rc = enter(ctx)) return rc;
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "no problem uploaded");
    if (int rc = ensure_csr(ctx)) return rc;
    const int64_t N = ctx->N, nz = 4 * ctx->nb;
    if (nnz) *nnz = nz;
    hipStream_t s = ctx->stream;
    if (rowptr || col) {
        HIPCHK(ctx->rp_full.reserve(4 * (2 * (size_t)N + 1)));
        HIPCHK(ctx->col_full.reserve(4 * (size_t)nz));
        magk::csr_export(ctx->bptr.as<int32_t>(), ctx->bcol.as<int32_t>(), N, ctx->rp_full.as<int32_t>(),
                         ctx->col_full.as<int32_t>(), s);
        HIPCHK(hipGetLastError());
        if (rowptr) HIPCHK(hipMemcpyAsync(rowptr, ctx->rp_full.p, 4 * (2 * (size_t)N + 1), hipMemcpyDeviceToHost, s));
        if (col) HIPCHK(hipMemcpyAsync(col, ctx->col_full.p, 4 * (size_t)nz, hipMemcpyDeviceToHost, s));
    }
    if (val) HIPCHK(hipMemcpyAsync(val, ctx->kval.p, 8 * (size_t)nz, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int mag_reduce_system(mag_ctx *ctx, int64_t *n_free, int64_t *nnz_ff, int32_t *rowptr, int32_t *col, double *val,
                      double *b)
{
    if (int rc = enter(ctx)) return rc;
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "no problem uploaded");
    if (int rc = ensure_csr(ctx)) return rc;
    const bool fill = rowptr || col || val || b;
    if (int rc = build_reduced(ctx, fill)) {
        if (n_free) *n_free = ctx->nf;
        if (nnz_ff) *nnz_ff = ctx->nz_ff;
        return rc;
    }
    const int64_t nf = ctx->nf, nz = ctx->nz_ff;
    if (n_free) *n_free = nf;
    if (nnz_ff) *nnz_ff = nz;
    hipStream_t s = ctx->stream;
    if (rowptr) HIPCHK(hipMemcpyAsync(rowptr, ctx->rp_ff.p, 4 * ((size_t)nf + 1), hipMemcpyDeviceToHost, s));
    if (col && nz) HIPCHK(hipMemcpyAsync(col, ctx->col_ff.p, 4 * (size_t)nz, hipMemcpyDeviceToHost, s));
    if (val && nz) HIPCHK(hipMemcpyAsync(val, ctx->val_ff.p, 8 * (size_t)nz, hipMemcpyDeviceToHost, s));
    if (b) HIPCHK(hipMemcpyAsync(b, ctx->b_ff.p, 8 * (size_t)nf, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAG_OK;
}

int mag_apply_operator(mag_ctx *ctx, const double *x, double *y, int32_t masked)
{
    if (ctx && ctx->field_on) return field_refuses(ctx, "mag_apply_operator");
    if (int rc = enter(ctx)) return rc;
    if (!ctx->have_problem) return fail(ctx, MAG_ERR_STATE, "no problem uploaded");
    if (!x || !y) return fail(ctx, MAG_ERR_BAD_ARGS, "null vector");
    if (int rc = ensure_full_order(ctx)) return rc;
    if (int rc = reserve_cg(ctx)) return rc;
    const int64_t N = ctx->N;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx->u.reserve(16 * (size_t)N));
    HIPCHK(hipMemcpyAsync(ctx->u.p, x, 16 * (size_t)N, hipMemcpyHostToDevice, s));
    magk::to_hilbert(ctx->u.as<double>(), ctx->iperm.as<int32_t>(), ctx->uknown.as<uint8_t>(), masked ? 1 : 0, N,
                     ctx->tmpP.as<double>(), s);
    if (int rc = apply_plain(ctx, ctx->tmpP.as<double>(), ctx->q.as<double>(), masked ? 1 : 0)) return rc;
    magk::from_hilbert(ctx->q.as<double>(), ctx->iperm.as<int32_t>(), N, ctx->u.as<double>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(y, ctx->u.p, 16 * (size_t)N, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ctx->have_run = false; // u was used as staging
    return MAG_OK;
}

int mag_time_operator(mag_ctx *ctx, int32_t reps, double *ms_per_launch)
{
    if (ctx && ctx->field_on) return field_refuses(ctx, "mag_time_operator");
    if (int rc = enter(ctx)) return rc;
    if (reps < 1 || !ms_per_launch) return fail(ctx, MAG_ERR_BAD_ARGS, "reps < 1 or null output");
    if (int rc = prepare_timing(ctx)) return rc;
    hipStream_t s = ctx->stream;
    if (ctx->fused) {
        if (int rc = reserve_fused(ctx)) return rc; // an on-chip solve leaves the streaming buffers unallocated
        // the fused iteration kernel on a scratch state that never reports convergence: dots {1,1,0,0}
        magk::FusedState h = {};
        h.jslot[0] = h.jslot[1] = 5;
        h.max_iter = (long long)1 << 60;
        HIPCHK(hipMemcpyAsync(ctx->fstate.p, &h, sizeof h, hipMemcpyHostToDevice, s));
        const int32_t stride = magk::kMaxGrid;
        HIPCHK(hipMemsetAsync(ctx->fpart.p, 0, 8 * 2 * 5 * (size_t)stride, s));
        const double one = 1.0;
        for (int c = 0; c < (ctx->pre ? 3 : 2); ++c) // {r.r, p.q[, rho]} = 1, the rest 0
            HIPCHK(hipMemcpyAsync(ctx->fpart.as<double>() + (size_t)c * stride, &one, 8, hipMemcpyHostToDevice, s));
        magk::FusedParams P = fused_params(ctx, 0);
        P.hist_len = 0;
        P.part_out = ctx->partRR.as<double>(); // scratch: keep {1,1,0,0} in place for every launch
        P.part_stride = 0;
        P.part_in = ctx->fpart.as<double>();
        P.part_stride_in = stride;
        P.nPart = 1;
        P.n_iface = 0;
        P.own_qslot = P.halo_qslot = nullptr; // single-GPU kernel: the figure is the operator's, not the exchange's
        P.comm_in_q = nullptr;
        P.comm_out_q = nullptr;
        return time_launches(ctx, reps, [&] { magk::fused_launch(P, ctx->B, ctx->fgrid, s); return 0; }, ms_per_launch);
    }
    // The CG buffers are free after a run: time the CG-mode operator kernel exactly as the solve launches it,
    // on a scratch state that never reports convergence.
    CgState h = {};
    h.rr_hist[0] = h.rr_hist[1] = 1.0;
    h.max_iter = (long long)1 << 60;
    HIPCHK(hipMemcpyAsync(ctx->state.p, &h, sizeof h, hipMemcpyHostToDevice, s));
    magk::OpParams P;
    magk::UpdParams U;
    iteration_params(ctx, 0, P, U);
    P.hist_len = 0;
    return time_launches(ctx, reps, [&] { magk::op_launch(P, ctx->B, true, s); return 0; }, ms_per_launch);
}

int mag_time_spmv(mag_ctx *ctx, int32_t reps, double *ms_per_launch)
{
    if (ctx && ctx->field_on) return field_refuses(ctx, "mag_time_spmv");
    if (int rc = enter(ctx)) return rc;
    if (reps < 1 || !ms_per_launch) return fail(ctx, MAG_ERR_BAD_ARGS, "reps < 1 or null output");
    if (int rc = prepare_timing(ctx)) return rc;
    // y = M K M v, nothing fused: the SpMV proper (tmpP holds a leftover vector of the run, q is free), on the tile
    // range this rank owns -- the whole mesh on one GPU, this GPU's share with several ranks
    return time_launches(
        ctx, reps, [&] { return apply_plain(ctx, ctx->tmpP.as<double>(), ctx->q.as<double>(), 1, true); }, ms_per_launch);
}

int mag_comm_get_unique_id(void *id_out) { return magc::get_unique_id(id_out); }

int mag_comm_init_rccl(mag_ctx *ctx, const void *unique_id, int32_t nranks, int32_t rank)
{
    if (int rc = enter(ctx)) return rc;
    std::string msg;
    const int rc = ctx->comm.init_rccl(unique_id, nranks, rank, ctx->stream, msg);
    if (rc) return fail(ctx, rc, "%s", msg.c_str());
    return MAG_OK;
}

int mag_comm_query(const mag_ctx *ctx, int32_t info[4])
{
    if (!ctx || !info) return MAG_ERR_BAD_ARGS;
    info[0] = ctx->comm.nranks;
    info[1] = ctx->comm.rank;
    info[2] = ctx->comm.nccl ? 1 : (ctx->comm.cb ? 2 : 0);
    info[3] = ctx->comm.rccl_count();
    return MAG_OK;
}

int mag_comm_set_window(mag_ctx *ctx, void *host_ptr, uint64_t bytes)
{
    if (int rc = enter(ctx)) return rc;
    if (ctx->win_host) {
        (void)hipHostUnregister(ctx->win_host);
        ctx->win_host = ctx->win_dev = nullptr;
        ctx->win_bytes = 0;
    }
    if (!host_ptr || bytes == 0) return MAG_OK; // window removed
    if (bytes < 4096) return fail(ctx, MAG_ERR_BAD_ARGS, "window of %llu bytes is too small", (unsigned long long)bytes);
    HIPCHK(hipHostRegister(host_ptr, (size_t)bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    void *dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dev, host_ptr, 0);
    if (e != hipSuccess) {
        (void)hipHostUnregister(host_ptr);
        return fail(ctx, MAG_ERR_HIP, "hipHostGetDevicePointer failed: %s", hipGetErrorString(e));
    }
    ctx->win_host = host_ptr;
    ctx->win_dev = dev;
    ctx->win_bytes = (size_t)bytes;
    return MAG_OK;
}

int mag_comm_inbox_create(mag_ctx *ctx, uint64_t bytes, void *handle_out)
{
    if (int rc = enter(ctx)) return rc;
    inbox_release(ctx);
    // whatever made an exchange through the OLD inboxes give up (another process on the GPU during a trial solve, a peer
    // that went away) says nothing about new ones
    ctx->si_failed = false;
    if (bytes == 0) return MAG_OK; // inboxes removed
    if (bytes < 4096 || !handle_out) return fail(ctx, MAG_ERR_BAD_ARGS, "inbox: %llu bytes / null handle", (unsigned long long)bytes);
    static_assert(sizeof(hipIpcMemHandle_t) == MAG_IPC_HANDLE_BYTES, "ipc handle size");
    // fine-grained: other GPUs' stores must become visible to this GPU's running kernel
    HIPCHK(hipExtMallocWithFlags(&ctx->inbox_own, (size_t)bytes, hipDeviceMallocFinegrained));
    HIPCHK(hipMemset(ctx->inbox_own, 0, (size_t)bytes));
    hipIpcMemHandle_t h;
    const hipError_t e = hipIpcGetMemHandle(&h, ctx->inbox_own);
    if (e != hipSuccess) {
        inbox_release(ctx);
        return fail(ctx, MAG_ERR_HIP, "hipIpcGetMemHandle failed: %s", hipGetErrorString(e));
    }
    memcpy(handle_out, &h, sizeof h);
    memcpy(ctx->inbox_handle.data(), &h, sizeof h);
    {
        std::lock_guard<std::mutex> lk(g_inbox_mu);
        g_inbox_here[ctx->inbox_handle] = ctx->inbox_own;
    }
    ctx->inbox_bytes = (size_t)bytes;
    return MAG_OK;
}

int mag_comm_inbox_open(mag_ctx *ctx, const void *handles)
{
    if (int rc = enter(ctx)) return rc;
    const int R = ctx->comm.nranks, me = ctx->comm.rank;
    if (!ctx->inbox_own || !handles || R < 2 || R > 8)
        return fail(ctx, MAG_ERR_STATE, "inbox_open needs mag_comm_inbox_create, a communicator of 2..8 ranks and the handles");
    for (int r = 0; r < R; ++r) {
        if (r == me) {
            ctx->inbox_peer[r] = ctx->inbox_own;
            continue;
        }
        hipIpcMemHandle_t h;
        memcpy(&h, (const uint8_t *)handles + (size_t)r * sizeof h, sizeof h);
        {
            std::array<uint8_t, MAG_IPC_HANDLE_BYTES> key;
            memcpy(key.data(), &h, sizeof h);
            std::lock_guard<std::mutex> lk(g_inbox_mu);
            const auto it = g_inbox_here.find(key);
            if (it != g_inbox_here.end()) { // that rank is a thread of this process
                ctx->inbox_peer[r] = it->second;
                ctx->inbox_peer_local[r] = true;
                hipPointerAttribute_t at;
                if (hipPointerGetAttributes(&at, it->second) == hipSuccess && at.device != ctx->device)
                    (void)hipDeviceEnablePeerAccess(at.device, 0); // already enabled is fine
                (void)hipGetLastError();
                continue;
            }
        }
        const hipError_t e = hipIpcOpenMemHandle(&ctx->inbox_peer[r], h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            ctx->inbox_peer[r] = nullptr;
            inbox_release(ctx);
            return fail(ctx, MAG_ERR_HIP, "hipIpcOpenMemHandle (rank %d) failed: %s", r, hipGetErrorString(e));
        }
    }
    ctx->inbox_ready = true;
    return MAG_OK;
}

int mag_comm_init_callback(mag_ctx *ctx, int32_t nranks, int32_t rank, mag_allreduce_fn fn, void *user)
{
    if (!ctx) return MAG_ERR_BAD_ARGS;
    std::string msg;
    const int rc = ctx->comm.init_callback(nranks, rank, fn, user, msg);
    if (rc) return fail(ctx, rc, "%s", msg.c_str());
    return MAG_OK;
}

} // extern "C"
