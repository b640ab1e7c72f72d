/*
 * magnetite_hip.h -- C ABI of the MI355X-native Magnetite solver hot path.
 *
 * This is the boundary a Rust `extern "C"` shim inside Magnetite's
 * `solver::run` binds (INTEGRATION.md shows the shim).  Every entry point
 * cites the reference interface it replaces (file:line into
 * kyle-tennison/Magnetite @ 2024_08_07).  Plain pointers and sizes only: no
 * C++ types, no exceptions, no torch types cross this boundary.
 *
 * Data model across the boundary (Rust `Vec<Node>` / `Option<f64>` are not
 * FFI-safe, so the shim flattens them -- datatypes.rs:1-29):
 *   xy[2N]       f64  node.vertex.{x,y}, interleaved              datatypes.rs:1-5
 *   conn[3E]     i32  element.nodes[0..3]                         datatypes.rs:17-18
 *   u_known[2N]  u8   1: node.ux/uy is Some (displacement prescribed, force unknown)
 *                     0: node.fx/fy is Some (force prescribed, displacement unknown)
 *   u_in[2N]     f64  prescribed displacement, read where u_known==1
 *   f_in[2N]     f64  prescribed force,        read where u_known==0
 *   DOF index    2*node + {0:x, 1:y}                              solver.rs:306-307,346-351
 * Every DOF has exactly one of (u,f) known -- the mesher guarantees it
 * (mesher.rs:615-624,881-900); the reference panics otherwise (solver.rs:431).
 * The shim checks it while flattening and reports MAG_ERR_BC_MISMATCH.
 *
 * Threading: one in-flight call per mag_ctx; calls block until the result is
 * complete; distinct contexts may be used from distinct threads.
 * Ownership: the caller owns every buffer it passes; the library keeps no
 * pointer after a call returns (device-resident inputs passed with
 * MAG_MEM_DEVICE are copied into context-owned buffers by mag_upload).
 * Errors: int status (0 == MAG_OK) + mag_last_error(); never aborts/throws.
 * The shim maps nonzero to MagnetiteError::Solver(msg) (error.rs:3-22).
 */
#ifndef MAGNETITE_HIP_H
#define MAGNETITE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAG_ABI_VERSION 4 /* 3: mag_stats gained exchange_timeout, best_param_mismatch; 4: edge_blocks (and, in the
                             reserved word behind it, tiles_per_workgroup).  Load cases (mag_set_load_cases ...
                             mag_get_cases_info) came later as new entry points only: no struct changed, the version
                             stays 4, and a caller detects the feature by the presence of those symbols (dlsym); design
                             variants (mag_set_variants ... mag_get_variants_info), sensitivities (mag_run_sensitivities,
                             mag_download_sensitivity), adjoint sensitivities (mag_run_adjoint ... mag_get_adjoint_info) and
                             mesh refinement (mag_run_refine ... mag_upload_refined), the element stiffness field
                             (mag_set_element_scale), the density design update (mag_design_init ... mag_download_design)
                             and the material law (mag_set_material_law, mag_get_material_law) likewise */

/* solver.rs:17-19 */
#define MAG_DOF 2
#define MAG_MAX_CG_ITER 10000000LL
#define MAG_TARGET_CG_COST 1e-4

typedef struct mag_ctx mag_ctx;

enum mag_status {
    MAG_OK = 0,
    MAG_ERR_BAD_ARGS = 1,
    MAG_ERR_BC_MISMATCH = 2,   /* no unknown displacement / inconsistent BC set (solver.rs:431 panics) */
    MAG_ERR_NOT_CONVERGED = 3, /* CG broke down: non-finite residual.  (The iteration cap is NOT an error: argmin's
                                  MaxItersReached is a normal termination and solver.rs:149-176 returns Ok(best_param);
                                  mag_run then returns MAG_OK with stats.converged = 0, stats.termination =
                                  MAG_TERM_MAX_ITERS and the lowest-cost iterate.  solver.rs:160-166 maps only an
                                  argmin Err, solver.rs:167-174 a missing best_param, to MagnetiteError::Solver.)   */
    MAG_ERR_HIP = 4,
    MAG_ERR_RCCL = 5,
    MAG_ERR_TOO_LARGE = 6,     /* an index would not fit int32                                   */
    MAG_ERR_STATE = 7          /* call order: no problem uploaded / not run yet                   */
};

/* CG stop rule.  argmin 0.10 reports cost = f(r.r) and the reference stops on the
 * ABSOLUTE threshold 1e-4 (solver.rs:153-154); whether f is sqrt or identity
 * cannot be verified offline, so both exist; default = the tighter. */
enum mag_stop {
    MAG_STOP_RNORM = 0,    /* sqrt(r.r) <= tol            (reference-compatible default) */
    MAG_STOP_RNORM_SQ = 1, /* r.r       <= tol                                            */
    MAG_STOP_REL = 2       /* sqrt(r.r) <= tol*sqrt(b.b)  (BASELINE config 3: "CG to 1e-8") */
};

/* Why the CG stopped (argmin's TerminationReason as the reference's Executor can produce it, solver.rs:149-157). */
enum mag_termination {
    MAG_TERM_NONE = 0,        /* no solve yet                                                              */
    MAG_TERM_TARGET_COST = 1, /* best_cost <= target_cost (solver.rs:154)                                  */
    MAG_TERM_MAX_ITERS = 2,   /* iter >= max_iters (solver.rs:153): the BEST iterate is returned            */
    MAG_TERM_BREAKDOWN = 3    /* non-finite residual (no reference counterpart: argmin would iterate on NaN) */
};

enum mag_operator {
    MAG_OP_MATRIX_FREE = 0, /* element-loop operator, K never read in the CG loop */
    MAG_OP_CSR = 1          /* reference-faithful: K_ff in CSR, solver.rs:31-36     */
};

/* Where a caller's arrays live.  One rule for every entry point and struct that carries a `memory`: a value that is none of
 * enum mag_memory is refused with MAG_ERR_BAD_ARGS, mag_last_error naming the function and mag_memory, among the argument checks
 * that precede any HIP call (so ahead of the MAG_ERR_STATE of a missing upload or run); where the pointers it describes are all
 * optional and NULL, so that nothing would be read or written through them, it is not looked at (an input that may be NULL:
 * mag_set_element_scale(NULL) clears, mag_run_refine's NULL indicator; output structs are always checked). */
enum mag_memory { MAG_MEM_HOST = 0, MAG_MEM_DEVICE = 1 };

typedef struct mag_options {
    int32_t device;       /* HIP device ordinal                                            */
    int32_t stop_mode;    /* enum mag_stop, default MAG_STOP_RNORM                         */
    double tol;           /* default MAG_TARGET_CG_COST (solver.rs:19)                     */
    int64_t max_iter;     /* default MAG_MAX_CG_ITER   (solver.rs:18)                      */
    int32_t cg_operator;  /* enum mag_operator, default MAG_OP_MATRIX_FREE                 */
    int32_t assemble_csr; /* 1 (default): build K in CSR as the reference does and take
                             the RHS and reactions from its rows; 0: matrix-free everywhere */
    int32_t check_every;  /* CG iterations per host convergence poll (default 64, even)    */
    int32_t use_graph;    /* 1 (default): replay the CG iteration block as a hipGraph      */
    int32_t tile_nodes;   /* owned nodes per workgroup tile: 256 | 512 | 1024; 0 (default): 512 for meshes of
                             >= 262144 nodes and for meshes of 32768..524288 nodes the on-chip CG can hold
                             (cg_variant 2), else 256                                       */
    int32_t history_len;  /* keep the cost of the first history_len iterations (tests)     */
    int32_t verbose;      /* 1: print the reference's "info:" phase lines to stdout        */
    int32_t op_variant;   /* 0 (default): LDS-halo operator when every tile fits LDS, else the
                             global-gather operator; 1: always the global-gather operator  */
    int32_t cg_variant;   /* One recurrence for 1 and 2 -- argmin's, with the numerator of beta, |r_new|^2, expanded
                             from exact dots of the previous iterate (r.r + 2 alpha r.q + alpha^2 q.q) so that one
                             grid-wide reduction per iteration suffices; alpha, the stop test and the reported
                             cost use the true r.r.
                             2 (default): on-chip -- when the whole mesh fits the registers and LDS of the chip
                               (about 0.5M nodes) the entire solve is ONE launch, the CG state never moves through
                               HBM, workgroups meet at a grid barrier once per iteration; otherwise as 1.
                             1: streaming -- one fused launch per CG iteration.
                             0: two launches per iteration, argmin's recurrences to the letter              */
    int32_t precision;    /* 0 (default): fp64 everywhere, as the reference.  1: the CG state, the operator and
                             (tile-relative) coordinates in fp32, dot products accumulated in fp64 -- the fp32
                             leg of BASELINE config 5's tolerance sweep; cannot meet the 1e-8 parity bar.  One GPU or
                             several (streaming protocol: one all-reduce per iteration, exchange buffer in doubles)  */
    int32_t preconditioner; /* 0 (default): plain CG, the reference's iteration (solver.rs:142).  OPT-IN ADDITION with
                             no reference counterpart: 1 Jacobi, 2 block-Jacobi on the 2x2 node-
                             diagonal blocks of K_ff (inverse blocks kept in fp32).  Same stop rule on the true
                             residual norm, same solution within the tolerance, fewer iterations on graded meshes.
                             Needs the fused LDS iteration (cg_variant 1, fp64, matrix-free operator).           */
    int32_t field_cg;     /* enum mag_field_cg: the CG under an element stiffness field (mag_set_element_scale); no effect
                             without one.  0 (default): the CSR operator's phase (mag_stats.cg_kernel 3).  OPT-IN: one fused
                             launch per iteration over the assembled K's block rows (cg_kernel 5) -- 1 plain CG, 2 Jacobi,
                             3 block-Jacobi on the 2x2 node-diagonal blocks of the scaled K_ff (inverse blocks in fp32).
                             `preconditioner` still refuses a field: the field's preconditioner is chosen here alone.
                             Falls back to the CSR operator's phase where the context has no tile-local tables
                             (mag_stats.lds_operator 0: op_variant 1, or a tile beyond LDS).  Other values read 0.
                             (this word was `reserved`: same offset, same size, zero means what it meant)           */
} mag_options;

enum mag_field_cg { MAG_FIELD_CG_CSR = 0, MAG_FIELD_CG_PLAIN = 1, MAG_FIELD_CG_JACOBI = 2, MAG_FIELD_CG_BLOCK_JACOBI = 3 };

/* Borrowed view of the caller's flattened Vec<Node>/Vec<Element>/ModelMetadata
 * (solver.rs:543-547 arguments). */
typedef struct mag_problem {
    int64_t num_nodes;
    int64_t num_elements;
    const double *xy;       /* 2N */
    const int32_t *conn;    /* 3E */
    const uint8_t *u_known; /* 2N */
    const double *u_in;     /* 2N */
    const double *f_in;     /* 2N */
    double youngs_modulus;  /* ModelMetadata, datatypes.rs:22-29; solver.rs:559-561 */
    double poisson_ratio;
    double part_thickness;
    int32_t memory; /* enum mag_memory: where the five arrays live */
    int32_t reserved;
} mag_problem;

/* Caller-allocated outputs: every node.ux,uy,fx,fy and element.stress becomes
 * Some(..) (solver.rs:476-482,532-533).  NULL members are skipped. */
typedef struct mag_result {
    double *u_out;      /* 2N */
    double *f_out;      /* 2N */
    double *stress_out; /* E  */
    int32_t memory;     /* enum mag_memory */
    int32_t reserved;
} mag_result;

typedef struct mag_stats {
    int64_t iterations; /* "finished conjugate gradient approximation in {} iterations", solver.rs:101-104 */
    double final_cost;  /* cost of the returned iterate under stop_mode */
    double rhs_norm;    /* sqrt(b.b) */
    int32_t converged;
    int32_t breakdown;  /* non-finite r.r */
    int64_t n_free;     /* unknown displacements */
    int64_t nnz;        /* scalar nnz of K (0 if not assembled) */
    int64_t num_tiles;
    int64_t ell_entries; /* (node,incident element) slots incl. padding */
    int64_t halo_nodes;  /* sum over tiles of nodes staged from other tiles */
    int32_t max_tile_halo;
    int32_t lds_operator; /* 1: LDS-halo operator ran, 0: global-gather fallback */
    int32_t cg_kernel;    /* what ran the CG: 0 two launches per iteration, 1 one fused launch per iteration,
                             2 on-chip single launch, 3 CSR operator, 4 fp32 leg, 5 one fused launch per iteration over
                             the assembled K's block rows (mag_options.field_cg, under an element stiffness field) */
    int32_t exchange;     /* several ranks, how they traded per iteration: 0 one rank, 1 one all-reduce (RCCL or the test
                             transport), 2 on-chip kernels through the inboxes, 3 streaming kernels through the inboxes */
    /* per-phase device time, HIP events on the context's stream, milliseconds */
    double ms_order;     /* Hilbert ordering + incidence + tile tables (symbolic, matrix-free op) */
    double ms_csr_symbolic;
    double ms_element;   /* K_e build, solver.rs:548-567 */
    double ms_assemble;  /* numeric gather into CSR, solver.rs:290-331 */
    double ms_bc;        /* RHS / partition, solver.rs:365-404,427-432 */
    double ms_cg;        /* solver.rs:435-441 timed region minus the dense->CSR scan */
    double ms_post;      /* scatter-back, reactions, stress */
    double ms_total;
    int64_t best_iteration; /* the iteration whose iterate is returned: argmin's best_param (solver.rs:167-174).  Equal to
                               `iterations` unless the solve stopped at the iteration cap                            */
    int32_t termination;    /* enum mag_termination */
    int32_t persist_timeout; /* 1: the on-chip CG kernel gave up at its grid barrier in this run (not every workgroup was
                               co-resident) and the streaming kernels redid the solve; the context then streams for a
                               number of solves (8, doubling after every further failure, at most 1024) before it tries
                               the on-chip kernel again */
    int32_t exchange_timeout; /* 1: several ranks, the inbox exchange of the streaming kernels gave up in this run and the
                                 ranks redid the solve with one all-reduce per iteration; the context keeps the all-reduce
                                 until its inboxes are created anew (mag_comm_inbox_create)                        */
    int32_t best_param_mismatch; /* iteration cap only: the iterate of `best_iteration` is recovered by repeating the
                                    solve up to that iteration; 1 when the repeat took another kernel or exchange than the
                                    first pass, or its cost there is not the recorded best cost bit for bit --
                                    `final_cost` is then the cost of the iterate actually returned                  */
    int32_t edge_blocks;    /* cg_kernel 2 only: 1 when the on-chip kernel ran its edge-block instantiation (every node's
                               triangles folded into at most six symmetric 2 x 2 blocks held in registers: meshes whose
                               nodes all carry one fan of at most six triangles, closed, or five, open); 2 when it ran the
                               edge-block instantiation WITH OVERFLOW (rows that are one fan of any length -- gmsh-type
                               meshes: the blocks beyond six per node in an LDS pool); 0 when it walked the
                               triangles (nodes with several fans, or a pool that does not fit)                     */
    int32_t tiles_per_workgroup; /* cg_kernel 2 only: tiles each workgroup of the on-chip kernel held (1-4 of 512 nodes; up
                                    to three on one GPU run the instantiation with that many node slots per lane)      */
} mag_stats;

/* ---- lifecycle ------------------------------------------------------- */
int mag_version(void);
void mag_default_options(mag_options *opt);
/* NULL opt => defaults.  Returns NULL only if the context itself cannot be allocated. */
mag_ctx *mag_create(const mag_options *opt);
void mag_destroy(mag_ctx *ctx);
const char *mag_last_error(const mag_ctx *ctx);

/* ---- the drop-in entry: replaces solver::run, solver.rs:543-586 ------ */
/* upload -> run -> download in one blocking call. */
int mag_solve(mag_ctx *ctx, const mag_problem *problem, mag_result *result);

/* The same, split so a caller (bench.py) can keep inputs resident in HBM:
 *   mag_upload   copies the problem into context-owned device buffers
 *   mag_run      K_e build, assembly, BC elimination, CG, reactions, stress (solver.rs:548-583)
 *   mag_download copies u/f/stress out */
int mag_upload(mag_ctx *ctx, const mag_problem *problem);
int mag_run(mag_ctx *ctx);
int mag_download(mag_ctx *ctx, mag_result *result);
int mag_get_stats(const mag_ctx *ctx, mag_stats *stats);
/* cost of CG iterations 1..n (n <= options.history_len, <= iterations) */
int mag_get_history(mag_ctx *ctx, double *history, int64_t n);

/* ---- load cases: several sets of prescribed values on ONE uploaded mesh ---- */
/* What a 2-D FEA user does with a part: solve it under several load sets.  Mesh, material and the u_known mask stay those
 * of mag_upload; only the VALUES change -- u_in where u_known == 1, f_in where u_known == 0.
 *   shared, done once per mag_run_cases: Hilbert order, tile tables, CSR pattern, K, the on-chip kernel's edge blocks;
 *   per case: right-hand side, CG, scatter-back, reactions, stress (solver.rs:365-533 per case).
 * When the mesh runs the on-chip CG (cg_variant 2, one GPU) and at least two cases fit the chip, the cases' CG solves run
 * side by side in one launch: G = the workgroups one case needs, floor(CUs / G) cases per launch, each case with its own
 * alpha, beta, stop test and iteration count.  Otherwise (a mesh of more than CUs / 2 workgroups, the fp32 leg, the CSR
 * operator, a preconditioner, cg_variant 0 / 1, a context backing off after an on-chip time-out) the cases' CG solves run one
 * after another through the single-case phases; the shared work is still done once.  Either way every case's u, f, stress
 * and CG statistics are BIT FOR BIT those of mag_upload + mag_run with that case's values.
 *
 * mag_set_load_cases: after mag_upload (whose own u_in / f_in mag_run_cases does not use).  u_in, f_in: [num_cases][2N],
 *   caller's DOF numbering, read as in mag_problem; copied into context-owned device buffers.  memory: enum mag_memory.
 *   A new mag_upload drops the cases.
 * mag_run_cases: MAG_OK when every case ended as mag_run's MAG_OK (the iteration cap included); otherwise the status of the
 *   first failing case (MAG_ERR_NOT_CONVERGED: a non-finite residual) -- the other cases are complete and can be downloaded.
 *   A case whose group of workgroups timed out at its barrier, or that stopped at the iteration cap with an earlier best
 *   iterate, is redone ONCE on its own through the single-case path (its time-out fall-back, its best_param repeat).
 *   options.history_len and options.verbose apply to case 0 only (mag_get_history then returns case 0's costs).
 *   mag_download / mag_get_stats of the single-case path hold nothing afterwards (mag_get_stats: case 0's statistics).
 * mag_get_case_stats: iterations, final_cost, rhs_norm, converged, breakdown, termination, best_iteration, cg_kernel,
 *   edge_blocks, tiles_per_workgroup, n_free, persist_timeout are the case's own; ms_cg is the time of the launch the case
 *   ran in (or of its own solve); ms_order, ms_csr_symbolic, ms_assemble (the shared work) and ms_bc, ms_post, ms_total (all
 *   cases together) are the same in every case.
 * mag_get_cases_info: info[0] cases, info[1] cases per on-chip launch (0: the cases ran one after another through the
 *   single-case CG phases), info[2] on-chip launches, info[3] cases redone on their own.
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS for num_cases < 1, a null pointer, a case index out of range, a context
 *   whose communicator has more than one rank (load cases across GPUs are not supported); MAG_ERR_STATE for
 *   mag_set_load_cases before mag_upload, mag_run_cases before mag_set_load_cases, mag_download_case / mag_get_case_stats /
 *   mag_get_cases_info before a completed mag_run_cases. */
int mag_set_load_cases(mag_ctx *ctx, int32_t num_cases, const double *u_in, const double *f_in, int32_t memory);
int mag_run_cases(mag_ctx *ctx);
int mag_download_case(mag_ctx *ctx, int32_t case_index, mag_result *result);
int mag_get_case_stats(const mag_ctx *ctx, int32_t case_index, mag_stats *stats);
int mag_get_cases_info(const mag_ctx *ctx, int32_t info[4]);

/* ---- design variants: several SHAPES and MATERIALS of one uploaded mesh (same connectivity, same u_known mask) ---- */
/* What shape optimisation, mesh morphing, tolerance / Monte-Carlo studies and sweeps of E, nu, thickness do: the topology stays,
 * node coordinates, the material and (optionally) the prescribed values change per variant.
 *   shared, done once per mag_run_variants: the Hilbert order OF THE UPLOADED COORDINATES, incidence, tile, ELL, ring and halo
 *     tables, masks, the CSR pattern, the on-chip kernel's instantiation (edge_blocks 0 / 1 / 2), overflow-pool layout and grid;
 *   per variant: permuted coordinates, K values in the shared pattern (bit for bit the reference's assembly for that geometry),
 *     right-hand side, edge blocks, CG, scatter-back, reactions (that variant's K), stress (its geometry, E, nu).
 * The variants' CG solves run side by side in the on-chip kernel by the load cases' rule -- floor(CUs / G) per launch, one
 * launch PER PHASE per chunk (permute, assemble, right-hand sides, blocks, CG, post), device memory bounded by one chunk's K --
 * when load cases would (and K is assembled: options.assemble_csr); otherwise one variant after another through the
 * single-case phases, the shared tables kept, the variant's coordinates and material swapped into the context.  Either way a
 * variant computes bit for bit what it computes as the only variant of a call of its own; a variant with the uploaded
 * coordinates computes bit for bit what mag_upload + mag_run compute with its material and values.
 *
 * mag_set_variants: after mag_upload.  xy [V][2N] or NULL (every variant keeps the uploaded coordinates); material [V][3] =
 *   E, nu, thickness or NULL (the uploaded material); u_in, f_in [V][2N] each or both NULL (the uploaded values).  At least one
 *   of the three must be given.  MAG_ERR_BAD_ARGS, with the first offender in mag_last_error: a material mag_upload would
 *   refuse; a variant in which an element's signed area differs in sign from the uploaded mesh's or is zero (the shared ring
 *   tables assume the uploaded orientation).  A refused material leaves the variants, their results and what was derived from
 *   them as they were, in either memory (values on the device are read back and checked before the set is touched); a refused
 *   shape has already replaced the set's coordinates, and the variants are gone.  A new mag_upload drops the variants.  Load cases and variants are independent
 *   sets of one context: setting or running one does not drop the other.
 * mag_run_variants, mag_download_variant, mag_get_variant_stats, mag_get_variants_info: as mag_run_cases ... mag_get_cases_info
 *   (status, the one redo of a variant whose group timed out or that stopped at the iteration cap with an earlier best iterate,
 *   history_len / verbose for variant 0 only, single-case results gone afterwards, info[0..3] = variants, per on-chip launch
 *   (0: one after another), launches, redone).  In a side-by-side run ms_element is the coordinate permutation, ms_assemble,
 *   ms_bc (right-hand sides and edge blocks) and ms_post the phases of all chunks together, ms_cg the variant's own launch.
 * Errors before any HIP call as for load cases; a context with more than one rank is refused. */
int mag_set_variants(mag_ctx *ctx, int32_t num_variants, const double *xy, const double *material, const double *u_in,
                     const double *f_in, int32_t memory);
int mag_run_variants(mag_ctx *ctx);
int mag_download_variant(mag_ctx *ctx, int32_t v, mag_result *result);
int mag_get_variant_stats(const mag_ctx *ctx, int32_t v, mag_stats *stats);
int mag_get_variants_info(const mag_ctx *ctx, int32_t info[4]);

/* ---- energy and design sensitivities of solved runs, load cases and variants ---- */
/* What shape optimisation and material sweeps need next to the solution: the objective -- strain energy, total potential energy
 * -- and its gradient with respect to the design, i.e. every node coordinate, E, nu and the thickness.  The problem is
 * self-adjoint: with prescribed displacements on the u_known DOFs and prescribed forces f on the others the potential is
 * Pi = 1/2 u^T K u - f_F^T u_F, at the solution dPi/du_F = 0, hence dPi/dtheta = 1/2 u^T (dK/dtheta) u -- no second solve.
 *   shared: the Hilbert order, the incidence lists and the tiles' halo lists of the uploaded mesh, as the set's run left them;
 *   per solved member: one pass over the elements, one over the nodes, one fixed-shape two-stage reduction -- launches of
 *     several members each (grid.y), chunked by a device-memory bound.
 * Everything follows the reference's K_e = (B^T D) B A t (solver.rs:263-278) with the SIGNED area A: a clockwise element gets
 * the sign that K_e gives it.
 *   energy[e]   = 1/2 u_e^T K_e u_e                                                                      (E values)
 *   dxy[2i + d] = sum over the triangles e of node i of 1/2 u_e^T (dK_e / dx_{i,d}) u_e, u held fixed      (2N values, caller
 *                 numbering; nodes with prescribed displacements included)
 *   scalars[0]  W = sum of energy[e]                         scalars[4]  dPi/dE  = W / E
 *   scalars[1]  Pi = W - scalars[2]                          scalars[5]  dPi/dnu = sum over e of 1/2 u_e^T (dK_e / dnu) u_e
 *   scalars[2]  external work: sum of f_in u over u_known == 0      scalars[6]  dPi/dt  = W / thickness
 *   scalars[3]  reaction work: sum of f_out u_in over u_known == 1  scalars[7]  0
 * dxy and scalars[4..6] are the TOTAL derivatives of Pi with respect to the design at fixed prescribed values.  For the
 * compliance C = f^T u over all DOFs that means: prescribed forces only (every prescribed displacement zero) C = -2 Pi, so
 * dC/dtheta = -2 dPi/dtheta -- stiffening the part lowers C --; prescribed displacements only (every prescribed force zero)
 * C = 2 Pi, so dC/dtheta = +2 dPi/dtheta.
 *
 * mag_run_sensitivities: set = enum mag_set.  Works on the results of the last completed mag_run / mag_run_cases /
 *   mag_run_variants, solves nothing and alters none of those results, whether the members ran side by side or one after
 *   another.  Every sum has a fixed order (no floating-point atomics): a repeat gives the same bits, and a member the same bits
 *   whatever launch it shares.  A new mag_upload, a new mag_set_* or a new run of the set drops the set's sensitivities.
 * mag_download_sensitivity: member `index` of the set (0 for MAG_SET_RUN); NULL arrays are skipped, scalars are always filled.
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS for a set that is none of enum mag_set, a negative or too large index, a null
 *   `out`, a context whose communicator has more than one rank; MAG_ERR_STATE for no completed run of the set and for
 *   mag_download_sensitivity before mag_run_sensitivities of it. */
enum mag_set { MAG_SET_RUN = 0, MAG_SET_CASES = 1, MAG_SET_VARIANTS = 2 };
typedef struct mag_sensitivity {
    double *energy_out; /* E,  NULL: skipped */
    double *dxy_out;    /* 2N, NULL: skipped */
    double scalars[8];
    int32_t memory;     /* enum mag_memory */
    int32_t reserved;
} mag_sensitivity;      /* 88 bytes */
int mag_run_sensitivities(mag_ctx *ctx, int32_t set);
int mag_download_sensitivity(mag_ctx *ctx, int32_t set, int32_t index, mag_sensitivity *out);

/* ---- adjoint sensitivities: the gradient of ANY objective of solved runs, load cases and variants ---- */
/* The potential energy above is the one self-adjoint objective.  Any other J(u) -- a displacement at a point, a target-shape
 * mismatch |u - u*|^2, a stress aggregate, a displacement constraint -- needs one more solve per member, with the member's own K:
 * member i of a solved set has u (all DOFs, prescribed values included) and K (its coordinates, E, nu, thickness); the caller
 * gives g = dJ/du (2N, caller numbering) evaluated at that u.  Split the DOFs into F (u_known == 0) and P (u_known == 1).  With
 * the prescribed values held fixed, K_FF u_F = f_F - K_FP u_P gives du_F/dtheta = -K_FF^-1 (dK/dtheta u)_F, hence with the adjoint
 *   K_FF lambda_F = g_F,   lambda_P = 0:        dJ/dtheta = g_F^T du_F/dtheta = -lambda^T (dK/dtheta) u.
 * Explicit partials (dJ/dtheta at fixed u) are the caller's to add.  Likewise dJ/df_F = K_FF^-1 g_F = lambda_F, and
 * dJ/du_P = g_P - K_PF lambda_F = g_P - (K lambda)_P, the second term being the reactions of the adjoint solve.
 * The bilinear form follows the reference's K_e with the SIGNED area, in the notation of the sensitivities: for a vector v
 *   p_v = sum b_i vx_i,  q_v = sum g_i vy_i,  r_v = sum (g_i vx_i + b_i vy_i),   A2 = 2A,  om = 1 - nu^2,
 *   Qb = p_l p_u + q_l q_u + nu (p_l q_u + q_l p_u) + (1 - nu) / 2 r_l r_u,      lambda_e^T K_e u_e = E t Qb / (2 A2 om),
 * and the coordinate and nu derivatives are its closed-form derivatives.  Per member:
 *   lambda      the adjoint solution, 0 on the prescribed DOFs                                          (2N values)
 *   dloads[i]   dJ/df_in[i] = lambda[i] where u_known == 0; dJ/du_in[i] = g[i] - (K lambda)[i] where u_known == 1  (2N values)
 *   delem[e]    -lambda_e^T K_e u_e: dJ with respect to a relative stiffness scale of element e -- what a density or
 *               thickness-field method consumes                                                        (E values)
 *   dxy[2i + d] -(sum over the triangles e of node i of lambda_e^T (dK_e / dx_{i,d}) u_e), nodes with prescribed
 *               displacements included                                                                  (2N values)
 *   scalars[0]  a = sum over e of lambda_e^T K_e u_e          scalars[2]  dJ/dnu = -(sum over e of lambda_e^T (dK_e / dnu) u_e)
 *   scalars[1]  dJ/dE = -a / E                                scalars[3]  dJ/dt  = -a / thickness;   scalars[4..7] = 0
 *
 * mag_run_adjoint: set = enum mag_set, after a completed run of that set; dJ_du [members][2N] (one row for MAG_SET_RUN), memory:
 *   enum mag_memory.  One objective per member per call: a second objective is a second call, which replaces the first's results.
 *   The adjoint systems are load sets (u_in = 0, f_in = g; entries of g on prescribed DOFs do not enter the solve) and run through
 *   the driver of the sets: for MAG_SET_RUN and MAG_SET_CASES as load cases -- K once, all members side by side, floor(CUs / G)
 *   per on-chip launch --, for MAG_SET_VARIANTS as variants with the set's coordinates and materials -- one launch per phase and
 *   chunk, device memory bounded by one chunk's K.  The fall-backs are the sets' (a mesh of more than CUs / 2 workgroups, the fp32
 *   leg, the CSR operator, a preconditioner, cg_variant 0 / 1, back-off): one member after another.  lambda of member i is BIT FOR
 *   BIT the u that mag_run_cases returns for the case (0, g_i) on the same upload, respectively mag_run_variants for that variant
 *   with the loads (0, g_i); mag_get_adjoint_stats / mag_get_adjoint_info (as mag_get_case_stats / mag_get_cases_info) report those
 *   solves.  The status follows mag_run_cases: the first failing member's, the others complete.
 *   STOP RULE: the adjoint solve stops by the context's rule like any case.  Under the two absolute rules (MAG_STOP_RNORM,
 *   MAG_STOP_RNORM_SQ) the accuracy of lambda therefore depends on the SCALE of g: a g of norm 1e-6 "converges" at once under an
 *   absolute 1e-4.  Scale the objective so that |g_F| is of the size of the primal right-hand side (mag_stats.rhs_norm), or use
 *   MAG_STOP_REL.
 *   Nothing else changes: the set's primal results, statistics and info words, its sensitivities, the other sets and -- although
 *   a set's run otherwise drops them -- mag_download, mag_get_stats, mag_get_history and the sensitivities of MAG_SET_RUN are bit for
 *   bit what they were.  The bilinear pass has no floating-point atomics: a repeat gives the same bits, a member the same bits
 *   whatever launch it shares.  A new mag_upload, a new mag_set_* of the set or a new run of the set drops the set's adjoint results
 *   (any set's run drops those of MAG_SET_RUN with the single-case results).
 * mag_download_adjoint: member `index` of the set (0 for MAG_SET_RUN); NULL arrays are skipped, scalars are always filled.
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS for a set that is none of enum mag_set, a null dJ_du / out / stats / info, an index
 *   out of range, a context whose communicator has more than one rank; MAG_ERR_STATE for no completed run of the set, and for
 *   download, stats or info before mag_run_adjoint of that set. */
typedef struct mag_adjoint {
    double *lambda_out; /* 2N, NULL: skipped */
    double *dloads_out; /* 2N */
    double *delem_out;  /* E  */
    double *dxy_out;    /* 2N */
    double scalars[8];
    int32_t memory, reserved;
} mag_adjoint;          /* 104 bytes */
int mag_run_adjoint(mag_ctx *ctx, int32_t set, const double *dJ_du /* [members][2N] */, int32_t memory);
int mag_download_adjoint(mag_ctx *ctx, int32_t set, int32_t index, mag_adjoint *out);
int mag_get_adjoint_stats(const mag_ctx *ctx, int32_t set, int32_t index, mag_stats *stats);
int mag_get_adjoint_info(const mag_ctx *ctx, int32_t set, int32_t info[4]); /* as mag_get_cases_info */

/* ---- objectives on the device: J, dJ/du and the explicit partials of solved runs, load cases and variants ---- */
/* mag_run_adjoint takes g = dJ/du from the caller and leaves J's explicit partials (dJ/dtheta at fixed u) to the caller.  For the
 * two objectives below the device forms both per solved member, where u lies, hands g to the adjoint pass without a copy to the
 * host, and adds explicit and adjoint parts to the total design gradient.  In the notation of the sensitivities (b, g, A2 = 2A
 * with the SIGNED area, p_u, q_u, r_u):
 * MAG_OBJ_STRESS_PNORM   the p-norm aggregate of the plane-stress von Mises stress.  sigma_e = D B u_e = (sx, sy, txy) with the
 *   reference's D (solver.rs:240-250) and B (solver.rs:204-230):  (sx, sy, txy) = E / ((1 - nu^2) A2) (P, Q, R),
 *   P = p_u + nu q_u, Q = nu p_u + q_u, R = (1 - nu) / 2 r_u;  vm_e = sqrt(sx^2 - sx sy + sy^2 + 3 txy^2).  (NOT the reference's
 *   scalar stress[e]: its sign factor (sx + sy < 1) is discontinuous.)
 *       S = sum_e w_e (vm_e / scale)^p,        J = scale S^(1/p),
 *   weights: E values >= 0, NULL for all ones; p >= 1 and scale > 0, both finite.  `scale` only keeps vm^p inside the range of
 *   a double: pass a typical stress of the part (the yield stress, the expected maximum); J does not depend on it but through
 *   round-off.  dJ/dz = S^(1/p - 1) / (2 scale) sum_e w_e (vm_e / scale)^(p - 2) d(vm_e^2)/dz; the explicit partials at fixed u:
 *   dJ/dxy is non-zero (B and A depend on the coordinates), dJ/dE = J / E, dJ/dnu in closed form from D, dJ/dt = 0.  An element
 *   with vm_e = 0 contributes 0 to S, to g and to the partials (for p < 2 its derivative does not exist); S = 0 gives J = 0,
 *   g = 0 and partials 0.
 * MAG_OBJ_DISP_LSQ       J = sum_i w_i (u_i - target_i)^2 over all 2N DOFs: weights 2N values >= 0 (required), target 2N values or
 *   NULL for zeros.  g = 2 w (u - target); every explicit partial is 0.  One non-zero weight is a displacement at a point, a
 *   target field a shape mismatch.
 * mag_objective: kind; per_member = 0: weights and target are ONE row for all members of the set, != 0: a row per member,
 *   [members][2N] (MAG_OBJ_DISP_LSQ) or [members][E] (MAG_OBJ_STRESS_PNORM); p and scale (MAG_OBJ_STRESS_PNORM only); memory: enum
 *   mag_memory of weights and target (rows on the device are read where they are).
 * mag_run_objective: set = enum mag_set, after a completed run of that set.
 *   with_adjoint = 0: nothing is solved; no other result of the context is touched.
 *   with_adjoint != 0: the device-resident g of all members goes through mag_run_adjoint's path -- its results for the set are
 *   those of mag_run_adjoint(set, g), bit for bit, readable through mag_download_adjoint, mag_get_adjoint_stats and
 *   mag_get_adjoint_info, and they REPLACE the results of an earlier adjoint call for the set; its status is returned (the first
 *   failing member's, the others complete).  Then total = explicit + adjoint, one addition per entry: dxy = pxy + the adjoint's dxy,
 *   dJ/dE, dJ/dnu, dJ/dt likewise.  The adjoint's STOP RULE caveat applies: under the absolute rules the accuracy of lambda depends
 *   on the scale of g, so scale the weights until |g_F| is of the size of mag_stats.rhs_norm (MAG_OBJ_DISP_LSQ: J and g are linear in w;
 *   MAG_OBJ_STRESS_PNORM: they grow with w^(1/p), so a factor c on g is a factor c^p on every weight), or
 *   use MAG_STOP_REL.
 *   Nothing else changes, as for mag_run_adjoint.  No floating-point atomics: a repeat gives the same bits, a member the same
 *   bits whatever launch it shares.  Objective results are dropped where the set's sensitivities are: a new mag_upload, a new
 *   mag_set_* of the set, a new run of the set (any set's run drops those of MAG_SET_RUN).
 * mag_download_objective: member `index` (0 for MAG_SET_RUN); NULL arrays are skipped, scalars are always filled:
 *   g_out        dJ/du                                                    (2N values, caller numbering)
 *   pxy_out      explicit dJ/dxy at fixed u                                (2N values)
 *   dxy_out      total dJ/dxy = pxy + adjoint dxy; with_adjoint only       (2N values)
 *   scalars[0]   J                      scalars[1..3]  explicit dJ/dE, dJ/dnu, dJ/dt
 *   scalars[4..6]  total dJ/dE, dJ/dnu, dJ/dt (0 without the adjoint)      scalars[7]  1 if the totals are present, else 0
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS for a set that is none of enum mag_set, an unknown kind, a null objective / out,
 *   a p or scale that is not finite or out of range, null weights for MAG_OBJ_DISP_LSQ, an index out of range, a context whose
 *   communicator has more than one rank; MAG_ERR_STATE for no completed run of the set, download before mag_run_objective of
 *   the set, and dxy_out when the objective ran with with_adjoint = 0. */
enum mag_objective_kind { MAG_OBJ_DISP_LSQ = 0, MAG_OBJ_STRESS_PNORM = 1 };
typedef struct mag_objective {
    int32_t kind;          /* enum mag_objective_kind */
    int32_t per_member;
    double p, scale;
    const double *weights;
    const double *target;
    int32_t memory, reserved;
} mag_objective;           /* 48 bytes */
typedef struct mag_objective_result {
    double *g_out;   /* 2N, NULL: skipped */
    double *pxy_out; /* 2N, explicit */
    double *dxy_out; /* 2N, total */
    double scalars[8];
    int32_t memory, reserved;
} mag_objective_result;    /* 96 bytes */
int mag_run_objective(mag_ctx *ctx, int32_t set, const mag_objective *objective, int32_t with_adjoint);
int mag_download_objective(mag_ctx *ctx, int32_t set, int32_t index, mag_objective_result *out);

/* ---- stress recovery: the tensor per element, the nodal field and the ZZ error estimate of solved runs, cases and variants ---- */
/* What a post-processor reads a part by, next to the reference-compatible scalar stress_out (which stays as it is): per solved
 * member the stress tensor of every element, a continuous nodal field for plots and read-outs at a point, and the
 * Zienkiewicz-Zhu estimate of the discretisation error -- whether the mesh that produced the stress can be trusted, and which
 * elements to refine.  In the notation of the sensitivities (b, g, A2 = 2A with the SIGNED area, p_u, q_u, r_u):
 *   (sx, sy, txy) = E / ((1 - nu^2) A2) (p_u + nu q_u, nu p_u + q_u, (1 - nu) / 2 r_u): sigma_e = D B u_e with the reference's D
 *                 and B; B carries 1 / A2, so the tensor is the physical one for either orientation of an element;
 *   vm            = sqrt(sx^2 - sx sy + sy^2 + 3 txy^2), MAG_OBJ_STRESS_PNORM's vm_e;
 *   elem[e]       = (sx, sy, txy, vm)                                                                  ([E][4] values)
 *   node[i]       = (sx*, sy*, txy*, vm(sigma*_i)) with the area-weighted average of the node's triangles
 *                   sigma*_i = (sum_{e of i} |A_e| sigma_e) / (sum_{e of i} |A_e|), the sums in the order of the node's
 *                   incidence list; caller numbering, nodes with prescribed displacements included, four zeros for a node
 *                   that no element touches                                                            ([N][4] values)
 *   eta2[e]       = |A_e| t / 12 (sum_k d_k^T C d_k + (sum_k d_k)^T C (sum_k d_k)),  d_k = sigma*_{n_k} - sigma_e for the three
 *                   corners, C = D^-1: s^T C s = (sx^2 - 2 nu sx sy + sy^2 + 2 (1 + nu) txy^2) / E -- the exact integral over the
 *                   triangle of (sigma* - sigma_e)^T C (sigma* - sigma_e) t with sigma* interpolated linearly and sigma_e
 *                   constant: what an adaptive mesher consumes                                          (E values)
 *   scalars[0]  eta^2 = sum of eta2[e]                        scalars[3]  the largest vm of the elements
 *   scalars[1]  U^2 = sum of |A_e| t sigma_e^T C sigma_e      scalars[4]  the largest vm(sigma*_i) of the nodes
 *               (= 2 |W| of the sensitivities)                 scalars[5..7]  0
 *   scalars[2]  eta_rel = sqrt(eta^2 / (U^2 + eta^2)), 0 where both are 0
 *
 * mag_run_stress: set = enum mag_set.  Works on the results of the last completed mag_run / mag_run_cases / mag_run_variants,
 *   solves nothing and alters no other result of the context -- primal results, statistics, sensitivities, adjoint and objective
 *   results of every set stay bit for bit --, whether the members ran side by side or one after another.  Every sum has a fixed
 *   order (no floating-point atomics): a repeat gives the same bits, and a member the same bits whatever launch it shares.  The
 *   recovery is dropped where the set's sensitivities are: a new mag_upload, a new mag_set_* of the set, a new run of the set (any
 *   set's run drops that of MAG_SET_RUN).
 * mag_download_stress: member `index` of the set (0 for MAG_SET_RUN); NULL arrays are skipped, scalars are always filled.
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS for a set that is none of enum mag_set, a negative or too large index, a null
 *   `out`, a context whose communicator has more than one rank; MAG_ERR_STATE for no completed run of the set and for
 *   mag_download_stress before mag_run_stress of it. */
typedef struct mag_stress_field {
    double *elem_out;  /* [E][4], NULL: skipped */
    double *node_out;  /* [N][4] */
    double *eta2_out;  /* [E]    */
    double scalars[8];
    int32_t memory, reserved;
} mag_stress_field;     /* 96 bytes */
int mag_run_stress(mag_ctx *ctx, int32_t set);
int mag_download_stress(mag_ctx *ctx, int32_t set, int32_t index, mag_stress_field *out);

/* ---- modal analysis: the lowest natural frequencies and mode shapes of the uploaded part -------------------
 * mag_run_modal: the `modes` lowest pairs of  K_FF phi_F = lambda M_FF phi_F,  phi_P = 0,  by subspace iteration on the device.
 *   Stiffness and supports.  K is the reference's stiffness of the uploaded mesh and material (solver.rs:263-331).  F is the set
 *     of DOFs with u_known == 0, P those with u_known == 1; prescribed DOFs are SUPPORTS: the uploaded u_in / f_in values play no
 *     role.
 *   Mass.  With density rho, m_e = rho * thickness * |A_e|.  Consistent (default): per direction M_e = m_e / 12 [[2,1,1],[1,2,1],
 *     [1,1,2]] on the element's three nodes; lumped (lumped != 0): m_e / 3 on each corner's diagonal.
 *   Orientation.  The reference's mesher guarantees counter-clockwise elements (check_ccw) and its K_e carries the signed area: a
 *     clockwise element makes K indefinite and inverse iteration meaningless.  A mesh with an element of signed area <= 0 is
 *     refused with MAG_ERR_BAD_ARGS, the first such element named in mag_last_error.
 *   Results, for modes = p:  lambda[k] ascending in (rad/s)^2;  frequency[k] = sqrt(lambda[k]) / (2 pi);  shape[k] (2N, caller
 *     numbering, 0 on P) normalised so that phi_k^T M phi_l = delta_kl, its entry of largest magnitude positive (on a tie the first
 *     in caller order);  residual[k] = |K_FF phi - lambda M_FF phi| / |lambda M_FF phi| from the pass's own quantities (below).
 *   A supported part is required: where too few supports leave a rigid-body motion free K_FF is singular, the inner CG breaks
 *     down or stalls and the call returns that status (MAG_ERR_NOT_CONVERGED).  There is no shift.
 * Algorithm: subspace iteration with q vectors, q = subspace or min(2p, p + 8) when 0;  p >= 1, p <= q <= 32, q <= n_free.
 *   1. q deterministic start vectors: DOF d of a node in vector j is a fixed integer hash of the bits of the node's coordinates
 *      and of 2 j + d, in [-1, 1), zero on P -- a function of the coordinates and j only, not of the numbering; independent on
 *      any mesh (a strip one element thick, where polynomials of the coordinates are exactly dependent, solves like any other
 *      part).  Y = M X.
 *   2. Each outer step: K_FF Z_j = Y_j for all q columns as ONE member set (u_in = 0, f_in = Y_j) through the driver of the load
 *      cases -- side by side on the chip, floor(CUs / G) per launch, where load cases run so, otherwise one after another;
 *      W = M Z;  A = Z^T Y (= Z^T K Z) and B = Z^T W, symmetrised;  on the host the pairs of (A, B), ascending, Q^T B Q = I,
 *      through the Cholesky factor of A scaled to a unit diagonal (A carries lambda_q / lambda_1 where B carries its square:
 *      slender parts and 32 vectors are within reach);
 *      X = Z Q, Y = W Q (K X = Y_old Q to the accuracy of the inner solves: no further operator application);
 *      residual[k] from Y_old Q e_k - lambda_k Y_new e_k.
 *   3. Stop when the largest relative change of the first p eigenvalues is <= tol, or after max_outer steps: reaching the cap is
 *      no error (converged = 0, the last iterate is returned, as with the CG's iteration cap).
 *   The inner solves run under MAG_STOP_REL with cg_tol whatever the context's stop rule is (its absolute rules mean nothing for
 *   right-hand sides of the size of a mass); the context's options are as they were afterwards.
 * mag_run_modal needs an uploaded problem, no run.  It alters no other result of the context: mag_download, mag_get_stats,
 *   mag_get_history, every set's results and every derived pass stay bit for bit.  Every sum has a fixed order: a repeat gives
 *   the same bits.  The modal results depend on the upload only: a new mag_upload drops them, a new mag_run_modal replaces them.
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS for a null pointer, modes < 1, subspace not 0 and outside [modes, 32] (or the
 *   default above 32), max_outer < 0, a density that is not positive and finite, a tol or cg_tol that is negative or not finite,
 *   an index out of range, a communicator of more than one rank; MAG_ERR_STATE for no upload and for mag_download_modal /
 *   mag_get_modal_info / mag_get_modal_stats before a completed mag_run_modal.  subspace > n_free: MAG_ERR_BAD_ARGS once the
 *   ordering phase has counted the free DOFs.
 * Errors of the iteration, all MAG_ERR_NOT_CONVERGED with mag_last_error naming mag_run_modal and the outer step; the earlier
 *   modal results are gone (MAG_ERR_STATE from mag_download_modal) and the context is usable as before: an inner solve that
 *   breaks down or stops at the iteration cap (its own words follow); a subspace whose vectors are linearly dependent -- a
 *   Cholesky pivot of the unit-diagonal A, or the ratio of the smallest to the largest eigenvalue of the reduced pencil, at or
 *   below 1e-13 --, the column and the figure named.  The hashed start vectors cannot be exactly dependent for a legal input;
 *   the tests' smallest figure is 1.4e-5 (an 8:1 cantilever, q = 20). */
typedef struct mag_modal_options {
    int32_t modes;      /* p >= 1 */
    int32_t subspace;   /* q, 0: min(2p, p + 8); p <= q <= 32 */
    int32_t max_outer;  /* 0: 50 */
    int32_t lumped;     /* 0 consistent mass, != 0 lumped */
    double density;     /* > 0, finite */
    double tol;         /* relative change of the first p eigenvalues; 0: 1e-10 */
    double cg_tol;      /* MAG_STOP_REL tolerance of the inner solves; 0: 1e-10 */
} mag_modal_options;    /* 40 bytes */
typedef struct mag_modal_result {
    double *lambda_out;    /* p, NULL: skipped */
    double *frequency_out; /* p */
    double *residual_out;  /* p */
    double *shapes_out;    /* [p][2N] */
    int32_t memory, reserved;
} mag_modal_result;        /* 40 bytes */
int mag_run_modal(mag_ctx *ctx, const mag_modal_options *opt);
int mag_download_modal(mag_ctx *ctx, mag_modal_result *out);
/* info[0] modes, [1] subspace, [2] outer steps, [3] converged, [4] vectors per on-chip launch (0: one after another),
 * [5] on-chip launches of all steps, [6] vectors redone alone, [7] 0 */
int mag_get_modal_info(const mag_ctx *ctx, int32_t info[8]);
/* statistics of inner solve j of the LAST outer step, as mag_get_case_stats */
int mag_get_modal_stats(const mag_ctx *ctx, int32_t j, mag_stats *stats);

/* ---- linearised buckling: the critical load factors and buckling shapes of a solved member ------------------------
 * mag_run_buckling: the `modes` pairs of smallest |lambda| of  (K_FF + lambda K_G,FF) phi_F = 0,  phi_P = 0,  on the device.
 *   Prestress.  u0 is the solution of a solved member: the last mag_run (set = MAG_SET_RUN, member 0) or case `member` of the
 *     last mag_run_cases (set = MAG_SET_CASES).  sigma_e = D B u0_e (plane stress, the uploaded material: mag_run_stress's
 *     tensor) and, with g_k the shape function gradients of the element,
 *       K_G,e[k, l] = t A_e (g_k^T sigma_e g_l) I_2.
 *   The classical linearised problem.  K is the stiffness at the reference configuration (mag_run_modal's); the
 *     initial-displacement terms of dK_T / dlambda are dropped.  lambda multiplies EVERYTHING prescribed in that member, forces
 *     and non-zero support displacements alike (u0 is linear in them).  Prescribed DOFs are supports, as in mag_run_modal.
 *   Orientation.  As mag_run_modal: an element of signed area <= 0 is refused with MAG_ERR_BAD_ARGS, the element named.
 *   Both signs are results.  A negative lambda is buckling under the reversed load; a pulled part has only such factors among its
 *     smallest.  load_factor[k], signed, is ordered by |lambda| ascending.  info[7] counts the positive ones among those returned.
 *   Results, for modes = p:  load_factor[k];  shape[k] (2N, caller numbering, 0 on P) normalised so that phi_k^T K phi_l =
 *     delta_kl (K_G is indefinite and cannot normalise), its entry of largest magnitude positive (on a tie the first in caller
 *     order);  residual[k] = |K_FF phi + lambda K_G,FF phi| / |lambda K_G,FF phi| from the pass's own quantities.
 * Algorithm: mag_run_modal's subspace iteration (one driver runs both) with -K_G in the place of M, so that it converges to the
 *   largest |mu|, mu = 1 / lambda;  q = subspace or min(2p, p + 8) when 0;  p >= 1, p <= q <= 32, q <= n_free.
 *   1. The same hashed start vectors X.  u0 is copied to a buffer of the pass.  Y = -K_G X, prescribed rows zero.
 *   2. Each outer step: K_FF Z_j = Y_j as ONE member set, as there;  W = -K_G Z;  A = Z^T Y (= Z^T K Z) and B = Z^T W,
 *      symmetrised;  on the host the pairs of B q = mu A q through the Cholesky factor of A scaled to a unit diagonal and cyclic
 *      Jacobi, ordered by |mu| descending, Q^T A Q = I (B is indefinite: nothing is factored but A);  lambda = 1 / mu;
 *      X = Z Q, Y = W Q;  residual[k] from Y_old Q e_k - lambda_k Y_new e_k.
 *   3. Stop when the largest relative change of the first p factors is <= tol, or after max_outer steps: reaching the cap is no
 *      error (converged = 0, the last iterate is returned).
 *   4. The shapes are K-normalised once more, by G = X^T (K_FF X) from one matrix-free product per shape: Z^T Y stands for
 *      Z^T K Z only as far as the inner solves reach K Z = Y.
 *   The inner solves run under MAG_STOP_REL with cg_tol, as mag_run_modal's.
 * mag_run_buckling alters no other result of the context: the run's and the cases' results, statistics and history, every
 *   derived pass and the modal results stay bit for bit.  A repeat gives the same bits.  The results stay until the next
 *   mag_upload or the next mag_run_buckling.
 * Errors, before the iteration: MAG_ERR_BAD_ARGS for a null pointer, modes < 1, subspace not 0 and outside [modes, 32] (or the
 *   default above 32) or above n_free, max_outer < 0, a tol or cg_tol that is negative or not finite, a set other than
 *   MAG_SET_RUN / MAG_SET_CASES, a member out of range, a communicator of more than one rank, a clockwise element;
 *   MAG_ERR_STATE for no upload, for a set that is not solved, for a context with an element stiffness field, for a download or
 *   query before a completed mag_run_buckling -- and for a prestress that VANISHES (a start column with -K_G x = 0, or an A_jj
 *   that is not positive at the first step): the chosen member carries no stress, there is nothing to buckle.
 * Errors of the iteration, all MAG_ERR_NOT_CONVERGED and named: an inner solve that breaks down or stops at its cap; a
 *   dependent subspace (column and figure named: a K_G of rank below `subspace` causes it, a smaller subspace helps); among the
 *   first p, a |mu_k| <= 1e-13 |mu_1|: fewer than p buckling modes exist.
 * Out of scope: a dead-load / live-load split; a shift (factors far from zero); variants as the prestress; fields; ranks; the
 *   prestress of a nonlinear state (K_T(u) of mag_run_newton as the first matrix); out-of-plane buckling (the model is a
 *   membrane). */
typedef struct mag_buckling_options {
    int32_t modes;      /* p >= 1 */
    int32_t subspace;   /* q, 0: min(2p, p + 8); p <= q <= 32 */
    int32_t max_outer;  /* 0: 50 */
    int32_t set;        /* MAG_SET_RUN or MAG_SET_CASES: whose solution is the prestress */
    int32_t member;     /* the case of MAG_SET_CASES; 0 for MAG_SET_RUN */
    int32_t reserved;
    double tol;         /* relative change of the first p factors; 0: 1e-10 */
    double cg_tol;      /* MAG_STOP_REL tolerance of the inner solves; 0: 1e-10 */
} mag_buckling_options; /* 40 bytes */
typedef struct mag_buckling_result {
    double *load_factor_out; /* p, NULL: skipped */
    double *residual_out;    /* p */
    double *shapes_out;      /* [p][2N] */
    int32_t memory, reserved;
} mag_buckling_result;       /* 32 bytes */
int mag_run_buckling(mag_ctx *ctx, const mag_buckling_options *opt);
int mag_download_buckling(mag_ctx *ctx, mag_buckling_result *out);
/* info[0] modes, [1] subspace, [2] outer steps, [3] converged, [4] vectors per on-chip launch (0: one after another),
 * [5] on-chip launches of all steps, [6] vectors redone alone, [7] positive factors among the modes returned */
int mag_get_buckling_info(const mag_ctx *ctx, int32_t info[8]);
/* statistics of inner solve j of the LAST outer step, as mag_get_case_stats */
int mag_get_buckling_stats(const mag_ctx *ctx, int32_t j, mag_stats *stats);
/* values_out = K_G(sigma(u0)) of the solved member (set, member as above) in the layout of mag_assemble_csr's val (its rowptr /
 * col apply; the off-diagonal entries of every 2 x 2 block are zero); memory: MAG_MEM_DEVICE for a device-resident values_out.
 * Every block is summed in the order of its row node's incidence list.  Alters no result of the context. */
int mag_assemble_geometric(mag_ctx *ctx, int32_t set, int32_t member, double *values_out, int32_t memory);

/* ---- transient dynamics: Newmark time stepping of the uploaded part, on the device ------------------------------
 * mag_run_transient: Newmark's method in acceleration form on the uploaded mesh and material, with density rho.
 *   Mass.  M is the consistent mass, or the lumped one (lumped != 0), as in mag_run_modal.  Damping: C = alpha M + eta K
 *     (rayleigh_mass, rayleigh_stiffness).
 *   Supports.  DOFs with u_known == 1 are supports held at the uploaded u_in for all time: u_P = u_in, v_P = a_P = 0.
 *   Loads.  The load on the free DOFs is amplitude[n] * f_in; amplitude is [steps + 1], NULL: all ones (a step load at t = 0).
 *   Start.  u_0, v_0 are given on F (2N vectors, their entries on P ignored), or zero.  M_FF a_0 = (amplitude[0] f - C v_0 - K u_0)_F.
 *   Step n -> n+1:   ut = u + dt v + dt^2 (1/2 - beta) a,   vt = v + dt (1 - gamma) a;
 *     A_FF a' = (amplitude[n+1] f - alpha M vt - K (ut + eta vt))_F,   A = (1 + gamma dt alpha) M + (beta dt^2 + gamma dt eta) K,   a'_P = 0;
 *     u' = ut + beta dt^2 a',   v' = vt + gamma dt a'.
 *     Prescribed displacements enter through K ut (ut_P = u_in): no elimination pass.
 *   beta and gamma are taken literally.  2 beta >= gamma >= 1/2 is unconditionally stable; anything else is the caller's to judge.
 *   The solves.  The initial solve and every step's are the same code with other coefficients ((c_M, c_K) = (1, 0) for a_0).  Each
 *     starts from zero and runs under MAG_STOP_REL with cg_tol whatever the context's stop rule is; the context's options are as
 *     they were afterwards.  An exactly zero right-hand side gives a' = 0 in 0 iterations.  cg: 0 fused block rows of A with
 *     block-Jacobi where the context has tile-local tables, else the CSR operator's phase; 1 | 2 | 3 fused plain / Jacobi /
 *     block-Jacobi; 4 the CSR operator's phase on A_FF.
 *   Reactions.  f_out is K (u + eta v) + M (a + alpha v) on P (the support reaction including inertia and damping) and
 *     amplitude[n] f_in on F.
 *   Records.  probes: DOF indices in caller numbering; their u, v, a at every step, row 0 = the start.  energies != 0: T = 1/2 v.Mv,
 *     W = 1/2 u.Ku, P = amplitude[n] f.u_F per step.  snapshot_every = k > 0: u at steps 0, k, 2k, ...
 *   resume != 0: starts from the final u, v, a, t of the previous completed run of this pass: no a_0 solve, u0 / v0 must be NULL,
 *     amplitude[0] is ignored.  Its records cover its own steps, row 0 the resumed state.  n1 steps followed by a resumed n2 steps
 *     give, bit for bit, the rows of one run of n1 + n2 steps.
 * mag_assemble_effective: c_K K + c_M M in the layout of mag_assemble_csr (values_out: 4 * blocks doubles in `memory`).
 * The pass needs an upload and no run.  It changes no other result of the context; a repeat gives the same bits (every sum has a
 *   fixed order, no floating-point atomics); a new mag_upload drops its results.
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS (mag_last_error naming the function and the argument) for a null struct, steps < 1,
 *   dt or density not positive and finite, beta, gamma, a Rayleigh coefficient or cg_tol negative or not finite, cg outside 0..4,
 *   snapshot_every < 0, num_probes < 0 or > 0 with NULL probes, a `memory` outside enum mag_memory, more than one rank;
 *   MAG_ERR_STATE for no upload, resume without a completed run or with u0 / v0, download or info before a completed run, a context
 *   with an element stiffness field (the message names the field), assemble_csr = 0 or precision = 1.
 * Errors after the first device work: a probe outside [0, 2N) and an element of signed area <= 0 (MAG_ERR_BAD_ARGS, the offender
 *   named, as mag_run_modal); records that would not fit device memory (MAG_ERR_TOO_LARGE); a solve that breaks down
 *   (MAG_ERR_NOT_CONVERGED naming the step: the pass's earlier results are gone, the context is usable as before).  The iteration
 *   cap is no error (info[7] = 0).
 * Out of scope: time-varying supports; a warm start of the step's CG; the on-chip CG on A; fields, variants and ranks; modal
 *   superposition. */
typedef struct mag_transient_options {
    int32_t steps, resume, lumped, cg, energies, snapshot_every, num_probes, memory;
    double dt, beta, gamma, density, rayleigh_mass, rayleigh_stiffness, cg_tol; /* cg_tol 0: 1e-10 */
    const double *amplitude, *u0, *v0;                                           /* NULL: ones, zero, zero */
    const int32_t *probes;                                                       /* NULL: none */
} mag_transient_options;                                                         /* 120 bytes */
void mag_default_transient_options(mag_transient_options *opt); /* beta 0.25, gamma 0.5, everything else 0 / NULL */
typedef struct mag_transient_result {
    double *u_out, *v_out, *a_out, *f_out;  /* 2N, the final state; NULL members are skipped */
    double *probe_u, *probe_v, *probe_a;    /* [steps + 1][num_probes], row 0 = the start */
    double *energies;                       /* [steps + 1][3] = T, W, P */
    double *snapshots;                      /* [steps / snapshot_every + 1][2N] of u, row 0 = the start */
    int32_t *iterations;                    /* [steps + 1], entry 0 = the a_0 solve (0 in a resumed run) */
    double scalars[4];                      /* t_start, t_end, 0, 0; after mag_run_explicit: t_start, t_end, the dt used, dt_bound
                                               (written by the call, on the host) */
    int32_t memory, reserved;
} mag_transient_result;                     /* 120 bytes */
int mag_run_transient(mag_ctx *ctx, const mag_transient_options *opt);
int mag_download_transient(mag_ctx *ctx, mag_transient_result *out);
/* info[0] steps done, [1] cg_kernel (3 or 5), [2] preconditioner (0 / 1 / 2), [3] CG iterations of all solves, [4] the largest of
 * a step, [5] snapshots kept, [6] resumed, [7] 1 when every solve converged */
int mag_get_transient_info(const mag_ctx *ctx, int32_t info[8]);
int mag_assemble_effective(mag_ctx *ctx, double c_K, double c_M, double density, int32_t lumped, double *values_out, int32_t memory);

/* ---- explicit dynamics: central-difference time stepping of the uploaded part, one fused launch a step -----------
 * mag_run_explicit: Newmark's method with beta = 0, gamma = 1/2 on the LUMPED mass m (mag_run_transient's lumped = 1), so that no
 *   system is solved: the method for impact, wave propagation and short shocks, where the step is bounded by the mesh's fastest
 *   mode anyway.  C = alpha M + eta K (rayleigh_mass, rayleigh_stiffness), the eta term taken at the half-step velocity.
 *   Supports, loads and the start are mag_run_transient's: u_P = u_in, v_P = a_P = 0; the load on F is amplitude[n] * f_in;
 *   u_0, v_0 given on F or zero.
 *   Start:  a_0 = (amplitude[0] f - alpha m v_0 - K (u_0 + eta v_0))_F / m   (the step below with dt = 0: one code).
 *   Step n -> n+1:   ut = u + dt v + dt^2/2 a,   vt = v + dt/2 a   (on P: ut = u_in, vt = 0);
 *     a' = (amplitude[n+1] f - alpha m vt - K (ut + eta vt))_F / ((1 + dt alpha / 2) m),   a'_P = 0;
 *     u' = ut,   v' = vt + dt/2 a'.
 *     With eta = 0 this is mag_run_transient(beta = 0, gamma = 0.5, lumped = 1) with its solve replaced by a division.
 *   The stable step.  lambda_bound = max over free DOFs i of (sum over free j of |K_ij|) / m_i (Gershgorin on M_FF^-1 K_FF),
 *     omega_bound = sqrt(lambda_bound), xi = eta omega_bound / 2, dt_bound = (2 / omega_bound) (sqrt(1 + xi^2) - xi): never above
 *     the true limit 2 / omega_max (and 0.69 - 0.94 of it on the test meshes).  The mass-proportional damping is centred in time
 *     and does not shrink the limit; the lagged stiffness-proportional part does.  dt = 0 asks for dt_scale * dt_bound (dt_scale 0:
 *     0.9).  A dt above dt_bound is NOT refused (the bound is conservative); a final state that is not finite is
 *     MAG_ERR_NOT_CONVERGED naming dt and dt_bound: the pass's results are gone, the context is usable as before.
 *   A step is ONE launch where the context has tile-local tables (info[2] = 1): the kernel reads K's tile-local block rows once,
 *     the state lives in Hilbert order in two buffers (a launch reads one and writes the other), amplitude[n + 1] is read on the
 *     device, and the host reads nothing between the launches.  The row order is a function of the mesh alone: the results are the
 *     same bits for every tile_nodes and every grid.  Without the tables (op_variant = 1, a tile beyond the LDS) a step is four
 *     launches in caller numbering (info[2] = 0), to the same accuracy.
 *   Records.  Probe and energy rows are written at steps 0, record_every, 2 record_every, ... (record_every 0: 1): steps /
 *     record_every + 1 rows; snapshots at steps 0, snapshot_every, ...  At such a step the state is moved to caller numbering and
 *     mag_run_transient's record kernels run; any other step is the one launch.
 *   Results.  The final u, v, a, t, the last amplitude and the reactions go into mag_run_transient's slots: mag_download_transient
 *     and mag_get_transient_info serve an explicit run (`iterations`: steps / record_every + 1 zeros), and either pass may resume
 *     the other's state.  n1 steps followed by a resumed n2 steps give, bit for bit, one run of n1 + n2 steps.
 * mag_explicit_dt: out[0] lambda_bound, [1] dt_bound with eta = 0, [2] dt_bound with rayleigh_stiffness, [3] the smallest node
 *   mass; needs an upload only.
 * Errors: mag_run_transient's rules, order and wording.  Before any HIP call: MAG_ERR_BAD_ARGS for a null struct, steps < 1, a dt,
 *   dt_scale or Rayleigh coefficient negative or not finite, a density not positive and finite, a negative record_every,
 *   snapshot_every or num_probes, num_probes > 0 with NULL probes, a `memory` outside enum mag_memory, more than one rank;
 *   MAG_ERR_STATE for resume with u0 / v0 or without a completed run, no upload, an element stiffness field, assemble_csr = 0 or
 *   precision = 1.  After the first device work: a probe outside [0, 2N), an element of signed area <= 0, records beyond device
 *   memory, the final state not finite.
 * Out of scope: several steps in one launch; a graph replay of the steps; time-varying supports; fields, variants and ranks; a
 *   sharper step estimate; element-wise step control, mass scaling, contact.
 *
 * kinematics = MAG_KIN_TOTAL_LAGRANGIAN: large rotations.  MAG_KIN_LINEAR (0, the default) is everything above, bit for bit.  With
 *   MAG_KIN_TOTAL_LAGRANGIAN the step is the one above with K (ut + eta vt) replaced by the internal force f_int(ut) of a
 *   St. Venant-Kirchhoff plane-stress material in the reference configuration.  For a triangle (a, b, c) with the reference edges
 *   db = X_b - X_a, dc = X_c - X_a and the relative displacements ub = u_b - u_a, uc = u_c - u_a:
 *     2A = db x dc;   H = grad u:   H11 = (dc.y ub.x - db.y uc.x) / 2A,   H12 = (db.x uc.x - dc.x ub.x) / 2A,
 *                                   H21 = (dc.y ub.y - db.y uc.y) / 2A,   H22 = (db.x uc.y - dc.x ub.y) / 2A;   F = I + H;
 *     Green-Lagrange strain  Exx = H11 + (H11^2 + H21^2) / 2,  Eyy = H22 + (H12^2 + H22^2) / 2,  Gxy = H12 + H21 + H11 H12 + H21 H22;
 *     second Piola-Kirchhoff stress, c = E / (1 - nu^2):  Sxx = c (Exx + nu Eyy),  Syy = c (Eyy + nu Exx),  Sxy = c (1 - nu) / 2 Gxy;
 *     first Piola-Kirchhoff stress P = F S;  the force on corner a is (t / 2) P (db.y - dc.y, dc.x - db.x)^T;
 *     the element's strain energy is W_e = A t (Sxx Exx + Syy Eyy + Sxy Gxy) / 2.
 *   Its linearisation at u = 0 is K, and a rigid motion u = (R - I)(X - X_c) + d gives zero force: a part may swing and whip.
 *     a' = (amplitude[n+1] f - alpha m vt - f_int(ut))_F / ((1 + dt alpha / 2) m).  Reactions: f_int(u) on P, amplitude[n] f on F.
 *     Energies: T = 1/2 v.mv, W = the sum of W_e, P = amplitude[n] f.u_F.  Supports, loads, the start (the step with dt = 0),
 *     records, resume and results are those above; either kinematics may resume the other's state, and a resumed run uses the
 *     kinematics it is given.
 *   rayleigh_stiffness must be 0 (MAG_ERR_BAD_ARGS otherwise): initial-stiffness damping is not objective.
 *   dt_bound stays the linear bound at the reference configuration, and dt = 0 asks for dt_scale times it.  Tension stiffens the
 *     part and shrinks the true limit: the caller lowers dt_scale for it.  The finite check on the final state is the safety net.
 *   An element with det F <= 0 is inverted.  It is no error: the run completes, info[7] is 0 and mag_last_error is unchanged.
 *   A step is ONE launch where the context has tile-local tables, and reads no matrix: the ring walk of the matrix-free operator
 *     with the force above per triangle.  A node's sum runs in its ring's order, which depends on tile_nodes: the same bits for
 *     every grid, a repeat and a resumed run, not across tile sizes.  Without the tables a step is four launches (info[2] = 0).
 *   Out of scope: plasticity, other hyperelastic laws; stiffness-proportional damping; an updated step bound during the run;
 *     follower loads; contact; fields, variants and ranks; several steps per launch.  (The implicit pass: mag_run_transient_tl.)
 * mag_internal_force: f_out = f_int(u) for all 2N DOFs in caller numbering (u, f_out: 2N doubles in `memory`), scalars_out[0] =
 *   W(u), scalars_out[1] = 1 if some element has det F <= 0, else 0 (written on the host).  The residual of a caller's own
 *   dynamic relaxation or Newton loop.  Needs an upload only and changes no result of the context; mag_run_explicit's refusals
 *   and wording (null u, f_out or scalars_out: MAG_ERR_BAD_ARGS). */
enum { MAG_KIN_LINEAR = 0, MAG_KIN_TOTAL_LAGRANGIAN = 1 };
typedef struct mag_explicit_options {
    int32_t steps, resume, energies, record_every, snapshot_every, num_probes, memory, kinematics; /* record_every 0: 1 */
    double dt, dt_scale, density, rayleigh_mass, rayleigh_stiffness;  /* dt 0: dt_scale * dt_bound; dt_scale 0: 0.9 */
    const double *amplitude, *u0, *v0;                                /* [steps + 1], 2N, 2N; NULL: ones, zero, zero */
    const int32_t *probes;                                            /* NULL: none */
} mag_explicit_options;                                               /* 104 bytes */
void mag_default_explicit_options(mag_explicit_options *opt); /* record_every 1, dt_scale 0.9, everything else 0 / NULL */
int mag_run_explicit(mag_ctx *ctx, const mag_explicit_options *opt);
/* after mag_run_explicit, mag_get_transient_info gives: info[0] steps done, [1] 6 (explicit), [2] 1 fused / 0 unfused, [3] step
 * launches (fused: steps + 1 with the start, steps in a resumed run; unfused: four per step), [4] record_every, [5] snapshots
 * kept, [6] resumed, [7] 1.  With MAG_KIN_TOTAL_LAGRANGIAN: [1] 7, [7] 0 when an element was inverted (det F <= 0) in some
 * evaluation of the force, 1 otherwise */
int mag_explicit_dt(mag_ctx *ctx, double density, double rayleigh_stiffness, double out[4]);
int mag_internal_force(mag_ctx *ctx, const double *u, double *f_out, double scalars_out[2], int32_t memory);

/* ---- nonlinear statics: Newton's method on the total-Lagrangian tangent, on the device ---------------------------
 * mag_run_newton: the large-deflection equilibrium of the uploaded part under the internal force above (MAG_KIN_TOTAL_LAGRANGIAN's
 *   f_int), in load increments.  Increment k = 1 .. increments has the load factor lambda_k = load_factors[k - 1], or
 *   k / increments where load_factors is NULL, and solves
 *     f_int(u)_F = lambda f_F on the free DOFs,   u_P = lambda u_in on the supports
 *   by Newton-Raphson with the consistent tangent of f_int.  Needs an upload and no run; changes no other result of the context.
 *   The tangent.  With H, F = I + H and S of the triangle as above, the reference shape gradients
 *     g_a = (db.y - dc.y, dc.x - db.x) / 2A,  g_b = (dc.y, -dc.x) / 2A,  g_c = (-db.y, db.x) / 2A  (cyclic shifts),
 *     V = A t,  D = c [[1, nu, 0], [nu, 1, 0], [0, 0, h]],  h = (1 - nu) / 2,
 *   the 2 x 2 block of corners (k, l) is
 *     K_T[k, l] = V (B_k^T D B_l + (g_k^T S g_l) I),   B_k (3 x 2) with column d = (F_d1 g_k.x,  F_d2 g_k.y,  F_d1 g_k.y + F_d2 g_k.x).
 *   K_T(0) = K.  It is assembled into K's pattern: block (i, j) is the sum over the triangles that hold i and j in the order of
 *   i's incidence list, without floating-point atomics: the same bits for a repeat, every grid and every tile_nodes.
 *   An iteration.  The first one of an increment moves the supports by its linearisation (the support predictor):
 *     dU_P = lambda u_in - u on P;   K_T,FF du_F = (lambda f - f_int(u))_F - (K_T dU_P)_F;   u += s (du_F + dU_P);
 *   the later ones solve K_T,FF du_F = (lambda f - f_int(u))_F with du_P = 0.  An iteration whose step the line search shortened
 *   (s < 1) leaves the supports short of lambda u_in: the next one is a first iteration again, on the rest of the way, until one
 *   with s = 1 has put them in place; an increment converges only then.  Every iteration is one evaluation of f_int, one
 *   tangent launch, the gather of the tangent into the solver's rows and one CG solve from zero under MAG_STOP_REL with cg_tol
 *   (0: 1e-10).  cg as mag_run_transient's: 0 block-Jacobi on the fused block-row kernel where the context has tile-local tables
 *   and the CSR operator's phase elsewhere, 1 | 2 | 3 the fused kernel plain | Jacobi | block-Jacobi, 4 the CSR operator's phase.
 *   Stop.  After every update: |r_F|_2 <= newton_tol * ref,  r = lambda f - f_int(u),  ref = max(|lambda f_F|_2, |f_int(u)_P|_2).
 *     newton_tol 0: 1e-10; max_newton 0: 25 iterations per increment.  The host reads one record of scalars per evaluation and
 *     the CG's convergence polls, nothing else.
 *   Line search.  line_search = H > 0: the step length s starts at 1 and is halved, at most H times, while the trial state
 *     u + s du has an inverted element (det F <= 0) or Pi(u + s du) > Pi(u) + 1e-4 s g, with Pi = W - lambda f_F.u_F and the slope
 *     g = (f_int(u) - lambda f_F).du (this is -r.du where du_P = 0).  The energy test is skipped where g >= 0 (a support predictor
 *     that works against the part) or |s g| <= 1e-13 max(|Pi|, W) (rounding).  H = 0 is plain Newton: s = 1.
 *   Not converged within max_newton: no error.  The run ends there; the state and the records stay at the last converged
 *     increment, info[7] is 0, info[0] the increments converged, and mag_last_error names the increment, the iteration and the
 *     ratio |r_F| / ref.  A CG that broke down (non-finite): MAG_ERR_NOT_CONVERGED naming increment and iteration, no results.
 *     An indefinite tangent (buckling, limit points) is out of scope: the CG needs K_T,FF positive definite.
 *   Start.  u0 (2N) starts from a given state: its P entries are where the supports stand.  NULL: zero.
 *   Records, row 0 the start and row k increment k: load (the factors, row 0: 0), probe_u (the load-deflection curve), energies
 *     (W, Pi), newton_iterations, snapshots (snapshots != 0).  residuals (|r_F| / ref after the update), cg_iterations and
 *     step_lengths have one entry per Newton iteration of the run: info[3] entries, at most increments * max_newton.  Rows of
 *     increments that did not converge are zero.
 *   Results: u_out (2N), f_out (2N: f_int on P, lambda f on F), elem (E x 8: Exx, Eyy, Gxy, Sxx, Syy, Sxy, det F, W_e).
 * mag_get_newton_info: info[0] increments converged, [1] cg_kernel (3 CSR operator's phase | 5 fused block rows), [2] preconditioner
 *   (0 none, 1 Jacobi, 2 block-Jacobi), [3] Newton iterations of the run, [4] CG iterations of the run, [5] halvings, [6] 1 when an
 *   element was inverted in an accepted state, [7] 1 when every increment converged.
 * mag_assemble_tangent: values_out = K_T(u) (u: 2N) in the layout of mag_assemble_csr's val (its rowptr / col apply).  Needs an
 *   upload only.
 * Errors: mag_run_transient's rules, order and wording.  Before any HIP call: MAG_ERR_BAD_ARGS for a null struct, increments < 1,
 *   a negative max_newton, line_search, num_probes, a newton_tol or cg_tol negative or not finite, cg outside 0..4, num_probes > 0
 *   with NULL probes, a `memory` outside enum mag_memory, more than one rank; MAG_ERR_STATE for no upload, an element stiffness
 *   field, assemble_csr = 0 or precision = 1.  After the first device work: an element of signed area <= 0, a probe outside [0, 2N).
 * Out of scope: arc-length and limit points; follower loads; plasticity, other hyperelastic laws; a warm-started or inexact inner solve; the on-chip
 *   CG on K_T; a matrix-free tangent operator; fields, variants and ranks.  (The implicit dynamic pass on the tangent:
 *   mag_run_transient_tl below.) */
typedef struct mag_newton_options {
    int32_t increments, max_newton, line_search, cg, snapshots, num_probes, memory, reserved;
    double newton_tol, cg_tol;
    const double *load_factors, *u0; /* [increments], 2N; NULL: k / increments, zero */
    const int32_t *probes;           /* NULL: none */
} mag_newton_options;                /* 72 bytes */
typedef struct mag_newton_result {
    double *u_out, *f_out, *elem;    /* 2N, 2N, E x 8 */
    double *probe_u, *snapshots;     /* [increments + 1][num_probes], [increments + 1][2N] */
    double *load, *energies;         /* [increments + 1], [increments + 1][2] */
    int32_t *newton_iterations;      /* [increments + 1] */
    double *residuals;               /* [info[3]] */
    int32_t *cg_iterations;          /* [info[3]] */
    double *step_lengths;            /* [info[3]] */
    int32_t memory, reserved;        /* NULL members are skipped */
} mag_newton_result;                 /* 96 bytes */
void mag_default_newton_options(mag_newton_options *opt); /* increments 1, everything else 0 / NULL */
int mag_run_newton(mag_ctx *ctx, const mag_newton_options *opt);
int mag_download_newton(mag_ctx *ctx, mag_newton_result *out);
int mag_get_newton_info(const mag_ctx *ctx, int32_t info[8]);
int mag_assemble_tangent(mag_ctx *ctx, const double *u, double *values_out, int32_t memory);

/* ---- nonlinear transient dynamics: Newmark steps, Newton's method on the total-Lagrangian tangent, on the device ----
 * mag_run_transient_tl: implicit dynamics with large rotations -- mag_run_transient's Newmark method in acceleration form with
 *   K u replaced by the internal force f_int(u) of MAG_KIN_TOTAL_LAGRANGIAN above, every step solved by Newton-Raphson with the
 *   consistent tangent K_T of mag_run_newton.  The step is not bound by the mesh's fastest mode: what mag_run_explicit with
 *   kinematics = MAG_KIN_TOTAL_LAGRANGIAN follows in hundreds of steps, this pass follows in one.
 *   Supports, loads, start, mass and records are mag_run_transient's: u_P = u_in, v_P = a_P = 0; the load on F is
 *   amplitude[n] f_in; the mass is consistent, or lumped; C = alpha M (rayleigh_mass).  There is no stiffness-proportional term
 *   (initial-stiffness damping is not objective) and no field for it.
 *     start   M_FF a_0 = (amplitude[0] f - alpha M v_0 - f_int(u_0))_F
 *     step    ut = u + dt v + dt^2 (1/2 - beta) a,   vt = v + dt (1 - gamma) a      (on P: ut = u_in, vt = 0)
 *             unknown a':  u' = ut + beta dt^2 a',   v' = vt + gamma dt a'
 *             r(a')   = (amplitude[n+1] f - f_int(u') - M (a' + alpha v'))_F
 *             Newton:  A_T,FF da = r_F,   A_T = (1 + gamma dt alpha) M + beta dt^2 K_T(u'),   a' += da
 *             first iterate:  a'_F = (u - ut)_F / (beta dt^2), so that u' = u_n (a zero displacement increment)
 *             stop, judged after every update:  |r_F|_2 <= newton_tol * ref,
 *                      ref = max(|amplitude[n+1] f_F|, |f_int(u')_F|, |(M (a' + alpha v'))_F|);  newton_tol 0: 1e-10;  max_newton 0: 25
 *     reactions   f_int(u) + M (a + alpha v) on P,  amplitude[n] f on F
 *     energies    T = 1/2 v.Mv,  W = the sum of the elements' W_e,  P = amplitude[n] f_F.u_F
 *   The first iterate is not a free choice.  a' = a_n and a' = 0 move the part by the linear predictor, which rotates it
 *     linearly and stretches it: at dt = T1 / 20 Newton then diverges or stalls on every case of the tests.  From u' = u_n it
 *     converges in 3 to 6 iterations a step.
 *   beta <= 0 is MAG_ERR_BAD_ARGS (beta = 0 leaves no system: that step is mag_run_explicit's); beta and gamma are otherwise taken
 *     literally.
 *   An iteration is: the effective tangent A_T in one launch (K_T's row walk, the lane that owns a row finishing it with c_M M; no
 *     K_T is kept), the gather of A_T into the solver's rows, one CG solve from zero under MAG_STOP_REL with cg_tol (0: 1e-10)
 *     through mag_run_transient's poll scheme, the state update, f_int, the residual with its norms.  The host reads one record of
 *     scalars per iteration and the CG's polls, nothing else.  cg = 0..4 selects as in mag_run_transient.
 *   Not converged within max_newton: no error, as mag_run_newton's increments.  The run ends there; the state and the records
 *     stay at the last converged step, MAG_OK is returned, mag_get_transient_tl_info's [7] is 0, [0] the steps done, and
 *     mag_last_error names the step, the iteration count and the ratio |r_F| / ref.  A CG that broke down (non-finite):
 *     MAG_ERR_NOT_CONVERGED naming step and iteration, no results.  An indefinite A_T is out of scope: the CG needs it positive
 *     definite (a small enough dt makes it so).
 *   An inverted element (det F <= 0) in a trial state raises info[6] and is no error.
 *   Results.  The final state, time, last amplitude, reactions and records go into mag_run_transient's slots:
 *     mag_download_transient and mag_get_transient_info serve the run (rows: steps done + 1; iterations[n]: the CG iterations of
 *     step n summed over its Newton iterations, entry 0 the a_0 solve; info[0] the steps done, [3] / [4] the CG iterations of all
 *     steps / the most of a step, [7] 1 when every step converged).  This pass, mag_run_transient and mag_run_explicit may each
 *     resume another's state; n1 steps and a resumed n2 give, bit for bit, one run of n1 + n2.
 * mag_get_transient_tl_info: info[0] steps done, [1] cg_kernel (3 | 5), [2] preconditioner, [3] Newton iterations of all steps,
 *   [4] the most of one step, [5] CG iterations of all solves (saturating), [6] 1 when an inverted element was seen, [7] 1 when
 *   every step converged.
 * mag_download_transient_tl: newton_iterations [steps done + 1] (entry 0 = 0); cg_iterations and residuals (|r_F| / ref after
 *   the update), one entry per Newton iteration of the run: info[3] entries; elem (E x 8, mag_run_newton's element rows of the
 *   final state).  NULL members are skipped.  Both need a completed mag_run_transient_tl that no other stepping pass has replaced.
 * mag_assemble_effective_tangent: values_out = c_K K_T(u) + c_M M in the layout of mag_assemble_csr's val, bit for bit
 *   mag_assemble_tangent's values combined with mag_assemble_effective's expression.  Needs an upload only.
 * The pass owns its matrix, table and work buffers: it changes no result of mag_run_newton, of a run, of a set or of
 *   mag_run_modal.  A repeat gives the same bits (every sum has a fixed order, no floating-point atomics).
 * Errors: mag_run_transient's rules, order and wording, the pass's own first: MAG_ERR_BAD_ARGS for a null struct, steps < 1, dt or
 *   density not positive and finite, beta negative, not finite or 0, gamma, rayleigh_mass, cg_tol or newton_tol negative or not
 *   finite, a negative max_newton, cg outside 0..4; then mag_run_transient's for the records, the context and the resume rule;
 *   after the first device work an element of signed area <= 0, a probe outside [0, 2N), records beyond device memory.
 * Out of scope: a line search; modified or quasi-Newton; a warm-started or inexact inner solve; stiffness-proportional damping;
 *   HHT / generalised-alpha; adaptive dt; time-varying supports; follower loads; plasticity, other hyperelastic laws; the on-chip CG on A_T; fields,
 *   variants and ranks. */
typedef struct mag_transient_tl_options {
    int32_t steps, resume, lumped, cg, energies, snapshot_every, num_probes, memory, max_newton, reserved;
    double dt, beta, gamma, density, rayleigh_mass, cg_tol, newton_tol; /* cg_tol, newton_tol 0: 1e-10; max_newton 0: 25 */
    const double *amplitude, *u0, *v0;                                   /* NULL: ones, zero, zero */
    const int32_t *probes;                                               /* NULL: none */
} mag_transient_tl_options;                                              /* 128 bytes */
typedef struct mag_transient_tl_result {
    int32_t *newton_iterations; /* [steps done + 1], entry 0 = 0; NULL members are skipped */
    int32_t *cg_iterations;     /* [info[3]] */
    double *residuals;          /* [info[3]] */
    double *elem;               /* E x 8 */
    int32_t memory, reserved;
} mag_transient_tl_result;      /* 40 bytes */
void mag_default_transient_tl_options(mag_transient_tl_options *opt); /* beta 0.25, gamma 0.5, everything else 0 / NULL */
int mag_run_transient_tl(mag_ctx *ctx, const mag_transient_tl_options *opt);
int mag_download_transient_tl(mag_ctx *ctx, mag_transient_tl_result *out);
int mag_get_transient_tl_info(const mag_ctx *ctx, int32_t info[8]);
int mag_assemble_effective_tangent(mag_ctx *ctx, const double *u, double c_K, double c_M, double density, int32_t lumped, double *values_out,
                                   int32_t memory);

/* ---- the material of the total-Lagrangian passes: St. Venant-Kirchhoff or compressible neo-Hooke -----------------
 * mag_set_material_law: the law that mag_run_explicit with kinematics = MAG_KIN_TOTAL_LAGRANGIAN, mag_internal_force,
 *   mag_run_newton, mag_assemble_tangent, mag_run_transient_tl and mag_assemble_effective_tangent read -- those six and nothing
 *   else.  It is context state like an option: MAG_LAW_SVK (0) by default, kept across mag_upload and mag_upload_refined, and
 *   setting it changes no stored result of any pass.  mag_get_material_law reads it back.  MAG_LAW_SVK is S = D E above, bit for
 *   bit: right for large rotations at strains of a few percent, wrong once a part is squeezed (its nominal stress in uniaxial
 *   compression peaks at stretch 0.577 and its tangent is indefinite beyond).
 * MAG_LAW_NEO_HOOKE: compressible neo-Hooke with the plane-stress condition enforced per element, on the upload's two constants
 *   mu = E / (2 (1 + nu)),  Lambda = E nu / ((1 + nu)(1 - 2 nu)).  With H, F = I + H, Exx, Eyy, Gxy, 2A, g_k and V = A t as above:
 *     energy       W = mu/2 (tr C + C33 - 3) - mu ln J + Lambda/2 (ln J)^2,   C = F^T F,  j2 = det C,  J^2 = j2 C33
 *     S33 = 0      mu (C33 - 1) + Lambda ln J = 0, a scalar equation for d = C33 - 1:
 *                  g(d) = mu d + Lambda/2 (log1p(j2m1) + log1p(d)) = 0,   j2m1 = j2 - 1 = 2 (Exx + Eyy) + 4 Exx Eyy - Gxy^2
 *                  g is increasing and concave (nu >= 0); Newton's method from d0 = min(0, -j2m1 / j2) starts at g <= 0 and rises
 *                  monotonically to the root: a counted loop, while the iterate still increases, of at most 40 iterations (at
 *                  most 15 over j2 = 1e-6 .. 1e6 and nu up to 0.499).  For nu < 0 g is convex and the iterates fall to the root
 *                  after the first step; the loop then runs while they fall.  u = 0 gives d = 0 exactly, nu = 0 gives d = 0 always.
 *     stress       S = mu (I - C33 C^-1), the Sxx, Syy, Sxy of the element rows
 *     force        on corner k:  V mu (F g_k - C33 h_k),  h_k = F^-T g_k  (= V F S g_k; exactly zero at u = 0)
 *     tangent      2 dS/dC = 2 mu C33 (kappa C^-1 (x) C^-1 + I_{C^-1}),  kappa = Lambda / (2 mu C33 + Lambda);  the block of corners
 *                  (k, l):  K_T[k, l] = V (mu (g_k . g_l) I + mu C33 (2 kappa h_k h_l^T + h_l h_k^T));  K_T(0) = K
 *     W_e          V W, from 2 (Exx + Eyy), d, log1p(j2m1) and log1p(d)
 *   A rigid motion gives zero force; the linearisation at u = 0 is K.
 *   An element with det F <= 0 raises the inverted flags exactly as under MAG_LAW_SVK, and nothing else is special-cased: det F < 0
 *     gives finite numbers from j2 = (det F)^2; det F = 0 gives non-finite ones, which the passes' existing checks catch (the line
 *     search rejects an inverted trial state; the finite checks on the final state and in the CG do the rest).
 *   rayleigh_stiffness, dt_bound and every other rule of the six entry points stay as they are.  dt_bound remains the linear bound at
 *     the reference configuration: neo-Hooke stiffens under compression as well as under tension, and the caller lowers dt_scale
 *     for either.  The three stepping passes may resume each other's state across laws (the state is u, v, a): a resumed run uses
 *     the law it finds.  A step stays one launch and a tangent one launch; every sum keeps its fixed order.
 * Errors: a law that is neither value: MAG_ERR_BAD_ARGS, the law stays.  Under MAG_LAW_NEO_HOOKE each of the six entry points
 *   refuses an upload with nu >= 0.5 or nu <= -1 with MAG_ERR_BAD_ARGS before any device work (the message names nu).
 * Out of scope: plasticity and other hyperelastic laws; the incompressible limit; the thickness stretch as an output; a step
 *   bound that follows the state. */
enum { MAG_LAW_SVK = 0, MAG_LAW_NEO_HOOKE = 1 };
int mag_set_material_law(mag_ctx *ctx, int32_t law);
int mag_get_material_law(const mag_ctx *ctx, int32_t *law);

/* ---- adaptive mesh refinement: longest-edge bisection with conformity closure (Rivara) of the uploaded mesh, on the device ----
 * What acts on the ZZ indicator of mag_run_stress: solve -> mag_run_stress -> mag_run_refine -> mag_upload_refined -> solve, the
 * mesh never leaving the device.  The reference (gmsh meshing, no adaptivity) has no counterpart.  The result is a pure function
 * of the inputs -- a repeat gives the same bits -- because the numbering is fixed:
 *   edges      local edge k of element e is (conn[3e + k], conn[3e + (k + 1) % 3]), identified by (lo, hi) = (smaller, larger
 *              node); its id is the rank of (lo, hi) in lexicographic order among the unique edges of the mesh;
 *   length     len2 = dx * dx + dy * dy with (dx, dy) = xy[hi] - xy[lo], two products and one addition, never fused: both
 *              elements of an edge see the same bits;
 *   longest    of an element: the local edge of largest len2, on a tie the smaller edge id -- a total order on the edges, which
 *              makes the closure terminate and the result conforming when lengths tie exactly;
 *   marked elements, by `rule`:
 *     MAG_REFINE_MARKS         marks[E], nonzero: marked;
 *     MAG_REFINE_MAX_FRACTION  ind[e] >= theta * max(ind), the product rounded once; nothing is marked when the maximum is 0;
 *     MAG_REFINE_TOP_FRACTION  the k = clamp(ceil(theta * E), 1, E) elements of largest indicator, ties to the lower element
 *                              index (a stable sort on the bits of ind[e] + 0.0);
 *     indicator: E values in `memory`, every one finite and >= 0 (otherwise MAG_ERR_BAD_ARGS, the first offender named in
 *     mag_last_error); NULL: the device-resident eta2 of the last mag_run_stress(MAG_SET_RUN), read where it lies.  theta in
 *     (0, 1].  No floating-point sum enters the marking;
 *   marked edges   split = 1: the longest edge of every marked element; split = 3: all three of its edges (Rivara's
 *              four-triangle variant: h halves where marked);
 *   closure    every element with a marked edge gets its longest edge marked, swept until a sweep marks nothing.  The marked set
 *              is the least fixed point.  A sweep reads the flags as they were before it, so the number of sweeps is the same in
 *              every run as well;
 *   new nodes  marked edge number r in edge-id order becomes node N + r at 0.5 * (x[lo] + x[hi]), 0.5 * (y[lo] + y[hi]).  Old
 *              nodes keep index, coordinates and boundary data.  Per DOF d of a new node: where u_known[2 lo + d] and
 *              u_known[2 hi + d] are both set, u_known = 1, u_in = 0.5 * (u_in[2 lo + d] + u_in[2 hi + d]); otherwise u_known = 0,
 *              u_in = 0; f_in = 0 always.  Point loads stay on their nodes, so the total load is preserved, and the constraint
 *              of the fine mesh interpolates the coarse one.  Re-stamping region rules (which put a force on EVERY node of a
 *              region, so the total would grow with the mesh) is the caller's: node_parents is there for that;
 *   new elements   an element without a marked edge is copied verbatim.  Otherwise, rotated so that its longest edge comes
 *              first, (p, q, r) with the new nodes M, A, B of pq, qr, rp: (p, M, B), (B, M, r) when rp is marked, else (p, M, r);
 *              then (M, q, A), (M, A, r) when qr is marked, else (M, q, r) -- 2, 3 or 4 children of the parent's orientation (a
 *              clockwise mesh stays clockwise).  The children of e occupy off[e] .. off[e + 1], off the exclusive scan of the
 *              child counts; elem_parent[E'] names each child's parent.
 * mag_run_refine: works on the uploaded mesh; MAG_REFINE_MARKS or a caller's indicator needs no run.  Solves nothing and alters
 *   no result of the context.  N' >= 2^30 or 9 E' >= 2^31: MAG_ERR_TOO_LARGE (mag_upload's limits).
 * mag_get_refine_info: info[0] N', [1] E', [2] elements marked before the closure, [3] marked edges (N' - N), [4] closure
 *   sweeps (the last, which marked nothing, included), [5] [6] [7] elements split in two, three, four.
 * mag_download_refine: NULL members are skipped.
 * mag_upload_refined: the refined mesh becomes the uploaded problem with the same material, copied device to device: bit for bit
 *   mag_download_refine followed by mag_upload, and like mag_upload it drops runs, sets and modes.  The refinement's arrays stay
 *   readable afterwards (the parents relate the new mesh to the old one) until a caller's mag_upload drops them or the next
 *   mag_run_refine replaces them.
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS for null options / info / out, an unknown rule, split not 1 or 3, a theta that is
 *   not finite or outside (0, 1] (rules 1 and 2), null marks under rule 0, a communicator of more than one rank; MAG_ERR_STATE
 *   before mag_upload, for a NULL indicator (rules 1 and 2) without a completed mag_run_stress(MAG_SET_RUN), and for info,
 *   download or mag_upload_refined before mag_run_refine.
 * Out of scope: refinement across ranks; of load-case or variant sets (the uploaded mesh and MAG_SET_RUN's indicator only);
 *   coarsening; snapping new boundary nodes to curved geometry (the model carries none); prolonging u as a starting guess (the
 *   solver takes none); carrying an element stiffness field over to the refined mesh (mag_upload_refined clears it). */
enum mag_refine_rule { MAG_REFINE_MARKS = 0, MAG_REFINE_MAX_FRACTION = 1, MAG_REFINE_TOP_FRACTION = 2 };
typedef struct mag_refine_options {
    int32_t rule;            /* enum mag_refine_rule */
    int32_t split;           /* 1 | 3 */
    double theta;            /* rules 1, 2: in (0, 1] */
    const uint8_t *marks;    /* rule 0: E */
    const double *indicator; /* rules 1, 2: E, NULL: eta2 of mag_run_stress(MAG_SET_RUN) */
    int32_t memory, reserved; /* enum mag_memory of marks and indicator */
} mag_refine_options;        /* 40 bytes */
typedef struct mag_refined {
    double *xy;            /* 2N', NULL: skipped */
    int32_t *conn;         /* 3E' */
    uint8_t *u_known;      /* 2N' */
    double *u_in, *f_in;   /* 2N' */
    int32_t *node_parents; /* [N' - N][2]: lo, hi of the edge a new node halves */
    int32_t *elem_parent;  /* [E'] */
    int32_t memory, reserved;
} mag_refined;             /* 64 bytes */
int mag_run_refine(mag_ctx *ctx, const mag_refine_options *opt);
int mag_get_refine_info(const mag_ctx *ctx, int64_t info[8]);
int mag_download_refine(mag_ctx *ctx, mag_refined *out);
int mag_upload_refined(mag_ctx *ctx);

/* ---- element stiffness field: a relative stiffness scale per element of the uploaded mesh ----
 * What a thickness field, a damaged region and a density (topology) method need: K = sum_e s_e K_e with K_e the reference's
 * element matrix (solver.rs:263-278) of the uploaded E, nu and thickness.  It is what mag_adjoint.delem differentiates.
 * mag_set_element_scale: after mag_upload.  scale: E values in `memory`, every one finite and > 0 (checked on the device:
 *   MAG_ERR_BAD_ARGS with the first offender named in mag_last_error, the field as it was); NULL clears the field, and the context
 *   computes bit for bit what it computed without one.
 *   Assembly: every contribution of element e to K is the value computed without a field, multiplied once by s_e, then added in
 *   the order it is added without a field (both assembly kernels carry the field as a template flag; without a field the
 *   kernels of a context without one run).  A field of all ones gives K bit for bit.
 *   What follows K follows the field: the right-hand side and the reactions (K's rows), mag_assemble_csr and mag_reduce_system
 *   (the scaled K).  mag_element_stiffness returns the UNSCALED K_e.
 *   Stress: stress_out[e] and MAG_OBJ_STRESS_PNORM stay functions of u, E and nu alone, sigma = D B u_e -- the stress of the
 *   unscaled material, which is the thickness-field and SIMP reading (a scale stands for less material carrying the same stress).
 *   CG: while a field is set the CG runs the CSR operator's phase whatever mag_options.cg_operator says (mag_stats.cg_kernel == 3):
 *   the on-chip kernel's edge blocks assume one material and the matrix-free operators carry no element id.
 *   Opt-in, mag_options.field_cg = 1 | 2 | 3: the CG runs one fused launch per iteration over the block rows of the assembled,
 *   scaled K instead (cg_kernel == 5; plain, Jacobi, 2x2 block-Jacobi), the rows' values gathered tile by tile after every
 *   assembly with the Dirichlet mask applied; where the context has no tile-local tables (lds_operator == 0) the CSR operator's
 *   phase runs as before (cg_kernel == 3).  The table of the rows is built in the first run and kept like the pattern.
 *   Load cases: mag_run_cases works under a field, K assembled once, the cases one after another (mag_get_cases_info: info[1] == 0);
 *   every case bit for bit mag_upload + mag_set_element_scale + mag_run of it.
 *   Passes: mag_run_sensitivities, mag_run_adjoint and mag_run_objective work for MAG_SET_RUN and MAG_SET_CASES; every element's term
 *   carries s_e:  energy[e] = s_e (1/2 u_e^T K_e u_e), hence dPi/ds_e = energy[e] / s_e;  delem[e] = -lambda_e^T (s_e K_e) u_e stays
 *   the derivative with respect to a RELATIVE scale, hence dJ/ds_e = delem[e] / s_e;  dxy and the scalars are sums of the scaled
 *   terms (dPi/dE, dPi/dt, dJ/dE, dJ/dt remain W / E ... of the scaled sums).
 *   Lifetime: mag_upload and mag_upload_refined clear the field.  Setting or clearing it drops the results of mag_run and
 *   mag_run_cases and everything derived from them; the Hilbert order, the tables and the CSR pattern of the first run under a
 *   field are kept by the runs that follow (mag_stats.ms_order == ms_csr_symbolic == 0 for them).
 * Refused with MAG_ERR_STATE before any HIP call, the message naming the field: while a field is set mag_set_variants,
 *   mag_run_variants, mag_run_modal, mag_run_stress, mag_run_refine, mag_apply_operator, mag_time_operator, mag_time_spmv, and the
 *   passes and their downloads for MAG_SET_VARIANTS (variants solved before the field was set carry none: their results stay and
 *   are readable again once the field is cleared); a field on a context
 *   with a communicator of more than one rank, assemble_csr = 0, precision = 1 or a preconditioner; mag_set_element_scale before
 *   mag_upload.  MAG_ERR_BAD_ARGS for a `memory` that is none of enum mag_memory (here and in mag_design_init, mag_design_step,
 *   mag_download_design). */
int mag_set_element_scale(mag_ctx *ctx, const double *scale /* E, or NULL: clear */, int32_t memory);

/* ---- density design update on the device: SIMP interpolation, a mesh-based density filter, the optimality-criteria update ----
 * mag_run -> mag_run_sensitivities -> mag_design_step -> mag_run ... iterates with the design never leaving the device; the order,
 * the tables and the CSR pattern are built once.  a_e is the signed area of element e (an element of area <= 0 is refused with
 * MAG_ERR_BAD_ARGS and named, as mag_run_modal does), P = filter_passes, p = penal.  Every sum has a fixed order (no floating-point
 * atomics): a repeat gives the same bits.
 *   filter F      n_i = (sum_{e in i} a_e x_e) / A_i,  A_i = sum_{e in i} a_e, both in the order of node i's incidence list;
 *                 (F x)_e = ((n_a + n_b) + n_c) / 3 with a, b, c in conn order: a one-ring radius on the tables stress recovery
 *                 averages over, no neighbour search;
 *   transpose     m_i = sum_{e in i} y_e / 3;  (F^T y)_e = a_e ((m_a / A_a + m_b / A_b) + m_c / A_c);
 *   interpolation rho~ = F^P rho,  s = scale_min + (1 - scale_min) rho~^p (repeated multiplication, no pow());
 *   chain rule    dJ/drho~_e = dJ/ds_e (1 - scale_min) p rho~_e^(p - 1),  dJ/drho = (F^T)^P dJ/drho~;
 *   volume        w = (F^T)^P a, once at init: the filtered volume sum_e a_e rho~_e is sum_e w_e rho_e, so the bisection filters
 *                 nothing;  target V* = volume_fraction sum_e a_e;
 *   OC update     Bq_e = max(-dJ/drho_e, 0) / w_e,
 *                 rho_new(L) = min(min(1, rho + move), max(max(rho_min, rho - move), rho sqrt(Bq / L)))  (fmin / fmax: where Bq / L
 *                 is 0 / 0 the lower limit stands),   V(L) = sum_e w_e rho_new_e(L);
 *   bisection     lo = 0, hi = max_e Bq_e / rho_min^2; exactly 100 times mid = 0.5 (lo + hi), lo = mid if V(mid) > V* else hi = mid;
 *                 the result is rho_new(0.5 (lo + hi)).  The bracket lives on the device: no read-back between the steps.
 * mag_design_init: after mag_upload.  rho0: E values in (0, 1] in `memory`, NULL: volume_fraction everywhere.  Stores rho, computes
 *   rho~ and s and installs s as the context's element scale, device to device, with mag_set_element_scale's effect on the
 *   context's results.  The scale is installed once everything is checked: a refused init (an element of area <= 0, a rho0
 *   outside (0, 1]) leaves a field of the caller's and the results under it as they were; a design in progress is ended.
 * mag_design_step: needs a completed mag_run under the installed scale.  dJ_ds: E values dJ/ds_e in `memory` for any objective (for
 *   instance delem / s of mag_run_adjoint), or NULL: the stiffest design, J = -2 Pi -- under prescribed forces C = -2 Pi, under
 *   prescribed displacements C = 2 Pi, so minimising J stiffens the part in both -- with dJ/ds_e = -2 energy[e] / s_e read from the
 *   device-resident energies of mag_run_sensitivities(MAG_SET_RUN), which it then needs.  Installs the new scale (the run is gone).
 * mag_get_design_info: info[0] volume fraction reached (sum_e w_e rho_e / sum_e a_e), [1] L, [2] max |rho_new - rho|, [3] greyness
 *   mean(4 rho~ (1 - rho~)), [4] 1 if V(lo0) >= V* >= V(hi0) (the target was reachable within the move limits), else 0 -- the step
 *   still returns MAG_OK with the nearest reachable design --, [5] steps since init, [6] J of the step (0 with a caller's gradient),
 *   [7] 0.  After mag_design_init: [0] and [3] of the start, the rest 0.
 * mag_download_design: NULL members are skipped; dJ_drho of the last step (zeros before the first).
 * mag_upload ends the design, and so does a mag_set_element_scale of the caller's.
 * Errors, before any HIP call: MAG_ERR_BAD_ARGS for null options / info / design and options outside their ranges; MAG_ERR_STATE
 *   for mag_design_init before mag_upload or on a context a field is refused on, mag_design_step before mag_design_init, before a
 *   completed mag_run, or with a NULL gradient before mag_run_sensitivities, and for info or download before mag_design_init.
 * Out of scope: the on-chip and fused CG under a field; fields for variants, modal analysis, stress recovery and refinement; more
 *   than one rank; non-integer penal, continuation schedules, MMA; passing delem to mag_design_step without a host round trip. */
typedef struct mag_design_options {
    double volume_fraction;   /* (0, 1] */
    double scale_min;         /* (0, 1), e.g. 1e-3 */
    double rho_min;           /* (0, 1) */
    double move;              /* (0, 1] */
    int32_t penal;            /* 1..8: rho^p by repeated multiplication, no pow() */
    int32_t filter_passes;    /* 0..8 */
    int32_t reserved[2];
} mag_design_options;         /* 48 bytes */
typedef struct mag_design {
    double *rho_out, *rho_filtered_out, *scale_out, *dJ_drho_out; /* E each, NULL: skipped */
    int32_t memory, reserved;
} mag_design;                 /* 40 bytes */
int mag_design_init(mag_ctx *ctx, const mag_design_options *opt, const double *rho0 /* NULL: volume_fraction everywhere */, int32_t memory);
int mag_design_step(mag_ctx *ctx, const double *dJ_ds /* E, or NULL: stiffness */, int32_t memory);
int mag_get_design_info(const mag_ctx *ctx, double info[8]);
int mag_download_design(mag_ctx *ctx, const mag_design *out);

/* ---- pieces of the path, exposed for parity tests -------------------- */
/* solver.rs:187-193 compute_element_area (pub; the mesher imports it, mesher.rs:9,523). Host-side. */
double mag_compute_element_area(const double *xy, const int32_t *tri);
/* solver.rs:204-230 compute_strain_displacement_matrix (pub): B[18], 3x6 row major, entries divided by 2*area. */
void mag_compute_strain_displacement_matrix(const double *xy, const int32_t *tri, double element_area, double *B);
/* solver.rs:240-250 compute_stress_strain_matrix (pub): D[9], 3x3 row major, plane stress. */
void mag_compute_stress_strain_matrix(double poisson_ratio, double youngs_modulus, double *D);
/* solver.rs:263-278 for every element of the uploaded problem: ke_out[36E] host, row-major 6x6.  Under an element stiffness field:
 * the UNSCALED K_e. */
int mag_element_stiffness(mag_ctx *ctx, double *ke_out);
/* solver.rs:290-331: K (2N x 2N) in CSR, ascending columns, structural pattern (under an element stiffness field: the scaled K,
 * here and in mag_reduce_system).
 * Call once with all outputs NULL to get nnz, then with host buffers rowptr[2N+1], col[nnz], val[nnz]. */
int mag_assemble_csr(mag_ctx *ctx, int64_t *nnz, int32_t *rowptr, int32_t *col, double *val);
/* The same for variant v of mag_set_variants (test only): K of that variant's coordinates and material in the pattern of the
 * uploaded mesh, assembled by the kernels mag_run_variants runs for a chunk. */
int mag_assemble_csr_variant(mag_ctx *ctx, int32_t v, int64_t *nnz, int32_t *rowptr, int32_t *col, double *val);
/* solver.rs:365-404,427-432,123-137: K_ff with exact zeros dropped + b, compact unknown numbering.
 * Same two-call pattern: rowptr[n_free+1], col[nnz_ff], val[nnz_ff], b[n_free]. */
int mag_reduce_system(mag_ctx *ctx, int64_t *n_free, int64_t *nnz_ff, int32_t *rowptr, int32_t *col,
                      double *val, double *b);
/* y = K x with the matrix-free element-loop operator on the uploaded mesh
 * (x, y: host, 2N, caller's DOF numbering).  masked != 0 applies M K M with M
 * zeroing prescribed-displacement DOFs (that is K_ff embedded in full length). */
int mag_apply_operator(mag_ctx *ctx, const double *x, double *y, int32_t masked);
/* y = M x with the mass operator of mag_run_modal (density, lumped as there) on the uploaded mesh (x, y: host, 2N, caller's
 * DOF numbering); masked != 0 applies P M P with P zeroing prescribed-displacement DOFs, as mag_apply_operator does (M_FF
 * embedded in full length).  Alters no result of the context. */
int mag_apply_mass(mag_ctx *ctx, double density, int32_t lumped, const double *x, double *y, int32_t masked);
/* y = K_G(sigma(u0)) x with the geometric stiffness operator of mag_run_buckling, u0 the solution of the solved member (set,
 * member as in mag_buckling_options) (x, y: host, 2N, caller's DOF numbering); masked != 0 applies P K_G P, as mag_apply_mass
 * does.  Reads no matrix.  Alters no result of the context. */
int mag_apply_geometric(mag_ctx *ctx, int32_t set, int32_t member, const double *x, double *y, int32_t masked);
/* Bench helper: `reps` back-to-back launches of the CG iteration kernel (cg_variant 1: the fused
 * iteration kernel; 0: the operator kernel of the two-launch iteration) on the context's stream
 * between two HIP events; *ms_per_launch = elapsed / reps.  Needs an uploaded problem, not a solve: straight after
 * mag_upload the symbolic phase is run and the vectors are zeroed.  With several ranks the launch covers the tiles
 * this rank owns (its per-GPU share). */
int mag_time_operator(mag_ctx *ctx, int32_t reps, double *ms_per_launch);
/* The same for the plain matrix-free SpMV y = M K M v (no CG update fused in). */
int mag_time_spmv(mag_ctx *ctx, int32_t reps, double *ms_per_launch);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------- */
#define MAG_UNIQUE_ID_BYTES 128
/* rank 0 calls this and broadcasts the bytes out of band (bench.py: torch.distributed) */
int mag_comm_get_unique_id(void *id_out);
int mag_comm_init_rccl(mag_ctx *ctx, const void *unique_id, int32_t nranks, int32_t rank);
/* What the context's communicator is: info[0] = ranks, info[1] = this rank, info[2] = transport (0 none, 1 RCCL,
 * 2 host callback), info[3] = ranks as RCCL itself reports them (ncclCommCount; 0 without an RCCL communicator). */
int mag_comm_query(const mag_ctx *ctx, int32_t info[4]);
/* test transport: sum-all-reduce of a host buffer supplied by the caller (gloo in tests/) */
typedef int (*mag_allreduce_fn)(void *user, double *host_buf, int64_t count);
int mag_comm_init_callback(mag_ctx *ctx, int32_t nranks, int32_t rank, mag_allreduce_fn fn, void *user);
/* EXPERIMENTAL multi-GPU on-chip CG (correct, but slower than the default once a rank has more than a few hundred
 * interface nodes: every granule is its own PCIe transaction -- see DESIGN.md): a window of HOST memory that every
 * rank of the node has mapped at `host_ptr` (the same
 * physical pages: POSIX shared memory, bytes >= 64 + 128 * nranks + 64 * interface nodes; a few MB is plenty).  With a
 * window and cg_variant 2 each rank runs its share of the mesh as ONE persistent launch and the per-iteration
 * exchange (one record of sums per rank, q of the interface nodes) goes through the window as tagged granules instead
 * of a collective per iteration; the communicator set by mag_comm_init_* is still used to line the launches up, to
 * agree on a fallback and to assemble the solution.  Without a window, or when the mesh does not fit the chips, the
 * streaming kernels + one all-reduce per iteration run.  NULL / 0 removes the window.  The window needs no preparation:
 * the extent a solve uses is cleared by rank 0 before the ranks line up, every solve. */
int mag_comm_set_window(mag_ctx *ctx, void *host_ptr, uint64_t bytes);
/* The same protocol with the window where it belongs: one INBOX per rank in that rank's device memory, mapped by the
 * other ranks through HIP IPC.  A rank only reads its own inbox (polls stay in local HBM); writers store into the
 * inboxes of the ranks that read a value (across xGMI).  Every rank: mag_comm_inbox_create(ctx, bytes, handle) (bytes
 * as for the window; `handle` receives MAG_IPC_HANDLE_BYTES bytes), exchange the handles by any means, then
 * mag_comm_inbox_open(ctx, all_handles) with the nranks handles in rank order.  bytes = 0 removes the inboxes.
 * When the mesh does not fit the chips the streaming kernels keep running one launch per iteration and trade through the
 * same inboxes between launches (mag_stats.exchange = 3) instead of one all-reduce per iteration.
 * Each rank's on-chip launch ends with one exchange workgroup (no tile: it gathers the rank's partial sums, trades them with the
 * other ranks through the inboxes and republishes the total) whenever a CU is free for it.
 * Exercised with up to eight ranks on ONE GPU only (~10 us per CG iteration with 8 ranks against ~40-90 through host
 * memory): measure before relying on it on a node, as bench.py does. */
#define MAG_IPC_HANDLE_BYTES 64
int mag_comm_inbox_create(mag_ctx *ctx, uint64_t bytes, void *handle_out);
int mag_comm_inbox_open(mag_ctx *ctx, const void *handles);

#ifdef __cplusplus
}
#endif
#endif /* MAGNETITE_HIP_H */
