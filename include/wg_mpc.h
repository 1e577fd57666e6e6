/*
 * wg_mpc.h -- C ABI of the MI355X-native ZMP-MPC hot path (libwg_mpc.so).
 *
 * Drop-in boundary for the per-tick inner loop of jrl-walkgen's Herdt-2010
 * pattern generator.  Plain pointers and sizes only; no C++/torch types.
 * Every entry point names the reference interface it replaces.
 *
 * Conventions
 *   - return value: 0 on success, negative on error (wg_last_error() has text);
 *   - per-QP `ifail` keeps the QL codes of the reference
 *     (src/privatepgtypes.hh:349-356): 0 ok, 1 too many iterations,
 *     2 accuracy insufficient, 5 workspace too short, >10 inconsistent
 *     constraints (10 + constraint code);
 *   - all matrices column-major (Fortran), one QP after the other, strides
 *     given by (nmax, mmax) exactly as ql0001_ takes them;
 *   - `_dev` variants take DEVICE pointers and a hipStream_t (passed as void*)
 *     and are asynchronous; the others take HOST pointers and are synchronous;
 *   - the library never falls back to a CPU path: without a usable HIP device
 *     every compute entry point fails with WG_ERR_NO_DEVICE.
 */
#ifndef WG_MPC_H
#define WG_MPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WG_OK 0
#define WG_ERR_NO_DEVICE (-1)
#define WG_ERR_BAD_ARG (-2)
#define WG_ERR_HIP (-3)
#define WG_ERR_TOO_LARGE (-4)
#define WG_ERR_BUSY (-5)      /* WG_OVERLAP_STRICT=1 only: a launch of the same context is still in flight on another stream */

/* Library / device management ------------------------------------------- */

/* Select the HIP device this process drives (one process per GPU). */
int wg_init(int device_ordinal);
void wg_shutdown(void);
const char *wg_last_error(void);
/* ABI version, bumped on any signature change. */
int wg_abi_version(void);
/* LDS bytes one QP of size (n, m) occupies in the solver kernel; lets callers
 * reason about occupancy (160 KiB per CU on gfx950). */
size_t wg_qp_lds_bytes(int n, int m);

/* Sharding (host arithmetic) ---------------------------------------------------------------------------------------------
 *
 * Gaits are independent (the reference has no coupling between pattern generators), so a fleet of `total` gaits is split
 * over `world` ranks -- one process per GPU -- by contiguous index range, the remainder spread over the first ranks:
 * rank r owns the global gaits [*lo, *hi).  Every rank derives per-gait inputs (seeds, references) from the GLOBAL index,
 * so the job's results do not depend on how it was split.  The only thing ranks exchange is the constant block
 * wg_model_t, which rank 0 broadcasts once (host/fleet_bench.cpp: ncclBroadcast; jrl-walkgen_amd/shard.py: the same
 * through torch.distributed). */
int wg_shard_range(long long total, int rank, int world, long long *lo, long long *hi);

/* Contexts ---------------------------------------------------------------------------------------------------------------
 *
 * Everything the library keeps between calls lives in a context: the configured models with the device copies of their
 * tables (wg_mpc_configure, wg_pldp_configure, wg_dimitrov_configure, wg_preview_configure), the per-launch workspaces of
 * the tick kernels (work queue of the multi-tick launch, per-block solver slots) and the staging buffers of the
 * host-pointer entry points.  The reference keeps the same things per object (one ZMPVelocityReferencedQP, one
 * PreviewControl ... per PatternGeneratorInterface); a context is what one such object owns here.
 *
 *   - every entry point NAME(args) below has a form NAME_ctx(ctx, args) with identical semantics on that context;
 *     NAME(args) itself works on a process-wide default context (device 0 unless wg_init chose another);
 *   - contexts are independent: two contexts may hold different models (N = 16 and N = 32, two robots, two preview
 *     windows) and their launches may overlap on different streams;
 *   - launches on ONE context share its workspaces: keep them on one stream (or order them with events).  Host-pointer
 *     entry points are synchronous and serialised per context: each context owns one non-blocking stream on which they copy
 *     in, launch and copy out, and they wait for THAT stream only -- never for the device: a host call on one context does
 *     not stall, and is not stalled by, the launches of another context or of the caller's own streams (two
 *     PatternGeneratorInterface objects, or a facade object beside a fleet, run side by side).  The same holds for the
 *     *_configure entry points: re-configuring waits for this context's earlier launches (their events), nobody else's;
 *   - a context belongs to one device; its entry points make that device current for the calling thread;
 *   - wg_ctx_destroy waits for the device, then frees everything the context owns. */
typedef struct wg_ctx wg_ctx_t;
int wg_ctx_create(int device_ordinal, wg_ctx_t **ctx);
void wg_ctx_destroy(wg_ctx_t *ctx);
int wg_ctx_device(const wg_ctx_t *ctx);
/* Launches of one context that arrive on different streams are ordered by the library (see wg_mpc_tick_batch_dev).  `on` != 0
 * makes the context refuse them instead (WG_ERR_BUSY); the initial value is WG_OVERLAP_STRICT of the environment, read once when
 * the context is created.  wg_overlap_serialised: how many launches of this context were ordered behind a launch of another
 * stream so far -- a caller that expected two streams to overlap reads its lost concurrency here (WG_OVERLAP_NOTE=1 in the
 * environment also prints one line to stderr at the first occurrence). */
int wg_set_overlap_strict(int on);
long long wg_overlap_serialised(void);

/* Batched dense QP solve -------------------------------------------------
 *
 * Replaces, batched over B independent problems,
 *     ql0001_(m, me, mmax, n, nmax, mnn, c, d, a, b, xl, xu, x, u, iout,
 *             ifail, iprint, war, lwar, iwar, liwar, eps1)
 *     src/Mathematics/qld.hh:27-31, called from QPProblem::solve
 *     src/ZMPRefTrajectoryGeneration/qp-problem.cpp:275-279
 * with iwar[0] = 1 (solver factorises the Hessian itself):
 *
 *     minimise  1/2 x'Cx + d'x   s.t.  A_j x + b_j  = 0  (j <  me)
 *                                      A_j x + b_j >= 0  (me <= j < m)
 *                                      xl <= x <= xu
 *
 *   B        number of QPs
 *   nmax     leading dimension of every C, stride of d/xl/xu/x/iact (>= max n)
 *   mmax     leading dimension of every A, stride of b             (>= max m)
 *   n,m,me   per-QP sizes, B ints each (n may be NULL => all nmax;
 *            m NULL => all mmax-1, the reference's convention m = mmax-1;
 *            me NULL => all 0)
 *   C        B * nmax*nmax     d, xl, xu   B * nmax
 *   A        B * mmax*nmax     b           B * mmax
 *   eps      the reference passes 1e-8 (qp-problem.cpp:260)
 * outputs
 *   x        B * nmax
 *   u        B * (mmax + 2*nmax): multipliers [general m | lower n | upper n]
 *            packed with the QP's own m and n like ql0001_'s u (may be NULL)
 *   ifail    B
 *   n_iter   B   ql0002's iteration counter                 (may be NULL)
 *   iact     B * nmax final active set in activation order, QL codes
 *            (1..m row, m+1..m+n lower bound, m+n+1.. upper), 0 padded
 *            -- what ql0001_ leaves in iwar[0..nact)          (may be NULL)
 *   nact     B                                               (may be NULL)
 *   hist     B * hist_cap add(+code)/drop(-code) log          (may be NULL)
 *   hist_len B   number of events (can exceed hist_cap)       (NULL iff hist NULL)
 * With more QPs than the device keeps resident, a batch that follows another one of the same size on the same C array starts
 * its QPs in the order of decreasing iteration count of that previous batch (an MPC loop: problem k of consecutive calls is
 * the same robot a tick later).  Scheduling only: no result depends on it; WG_QL_LPT=0 keeps index order. */
int wg_qp_solve_batch(int B, int nmax, int mmax, const int *n, const int *m,
                      const int *me, const double *C, const double *d,
                      const double *A, const double *b, const double *xl,
                      const double *xu, double eps, double *x, double *u,
                      int *ifail, int *n_iter, int *iact, int *nact, int *hist,
                      int hist_cap, int *hist_len);

int wg_qp_solve_batch_dev(int B, int nmax, int mmax, const int *n, const int *m,
                          const int *me, const double *C, const double *d,
                          const double *A, const double *b, const double *xl,
                          const double *xu, double eps, double *x, double *u,
                          int *ifail, int *n_iter, int *iact, int *nact,
                          int *hist, int hist_cap, int *hist_len,
                          void *hip_stream);


/* ------------------------------------------------------------------------
 * Herdt-2010 MPC tick, batched over independent gaits
 *
 * One "tick" = one execution of the body of
 *     ZMPVelocityReferencedQP::OnLine            (ZMPVelocityReferencedQP.cpp:346-452)
 * for one gait: support-state preview, orientation preview, QP assembly,
 * QL solve, LIPM interpolation + state step, trunk and feet interpolation.
 * The reference keeps this state in C++ objects and four deques; here it is a
 * flat POD per gait so that B gaits sit in one HBM array.
 * ---------------------------------------------------------------------- */

/* FootAbsolutePosition without time/stepType (include/jrl/walkgen/pgtypes.hh:137-154);
 * x,y,z in metres, angles in DEGREES like the reference. */
typedef struct wg_foot_sample {
  double x, y, z, theta, omega, omega2;
  double dx, dy, dz, dtheta, domega, domega2;
  double ddx, ddy, ddz, ddtheta, ddomega, ddomega2;
} wg_foot_sample_t;

enum { WG_LEFT = 0, WG_RIGHT = 1 };   /* foot_type_e, privatepgtypes.hh:47-50 */
enum { WG_SS = 0, WG_DS = 1 };        /* PhaseType,   privatepgtypes.hh:65-68 */

/* Robot / algorithm constants (what the path reads from CjrlHumanoidDynamicRobot
 * plus the constants hard-coded in the reference's constructors). */
typedef struct wg_model {
  int N;                    /* QP_N_ = 16            ZMPVelocityReferencedQP.cpp:64  */
  int flags;                /* WG_FLAG_* below */
  double T;                 /* QP_T_ = 0.1                                     :63  */
  double Tctrl;             /* m_SamplingPeriod = 0.005                        :65  */
  double com_height_qp;     /* 0.814                                      :103,114  */
  double alpha, beta, gamma;/* 1.0, 1e-5, 1e-6 (INSTANT_VELOCITY, JERK_MIN, COP_CENTERING) :116-118 */
  double sole_w, sole_h;    /* CjrlFoot::getSoleSize outputs, relative-feet-inequalities.cpp:158-172 */
  double margin_x, margin_y;/* 0.04, 0.04                                      :48-49 */
  double ds_feet_distance;  /* 0.2                                             :47   */
  double hip_l_lo, hip_l_hi, hip_r_lo, hip_r_hi; /* hip-yaw limits, OrientationsPreview.cpp:42-66 */
  double hip_vmax;          /* |upperVelocityBound|                            :68   */
  double hip_amax;          /* 0.1                                             :71   */
  double feet_cross_max;    /* 5 deg in rad                                    :73   */
  double step_period;       /* 0.8   SupportFSM, ZMPVelocityReferencedQP.cpp:76.  The tick holds at most four previewed
                             * steps: with k = ceil((step_period - T/10 - 1e-6) / T) previewed instants between two support
                             * changes, wg_mpc_configure refuses (WG_ERR_BAD_ARG) a model with 1 + (N - 2) / k > 4
                             * (T = 0.1: step_period <= 0.71 at N = 32, <= 0.31 at N = 16) */
  double ds_period;         /* 1e9                                             :77   */
  double dsss_period;       /* 0.8                                             :78   */
  double t_single;          /* 0.7   rigid-body-system.cpp:60                        */
  double t_double;          /* = T   rigid-body-system.cpp:61                        */
  double step_height;       /* 0.05  rigid-body-system.cpp:66                        */
  double feet_distance;     /* 0.2   rigid-body-system.cpp:65                        */
} wg_model_t;

/* wg_model_t.flags */
#define WG_FLAG_NO_STOP_CENTERING 1  /* skip the "go to the feet centre when NbStepsLeft == 0" branch
                                        (ZMPVelocityReferencedQP.cpp:410-421).  That branch was added
                                        after the reference's golden .datref was recorded (ChangeLog
                                        [3.1.8] "Put the CoM at the center of the feet when stopping");
                                        the flag exists so the golden file can be replayed. */
/* Where wg_mpc_configure takes the invariant Hessian block Q_b = beta I + alpha Uv'Uv + gamma Uz'Uz from
 * (GeneratorVelRef::build_invariant_part, generator-vel-ref.cpp:587-614).  Default (neither flag): the host loop in the
 * reference's summation order -- the tick is then bit-exact.  With a flag: the matrix cores (wg_gramian_batch), in fp64
 * (entries equal to rounding, 1e-14) or in fp32 (operands rounded to float: BASELINE's "fp32, MFMA Gramian condensation
 * path"; entries to 8e-8 of the largest one, which moves the jerk solution by ~1e-3 relative at N = 32 because Q_b's
 * smallest eigenvalue is beta = 1e-5 -- a tolerance mode, not a parity mode). */
#define WG_FLAG_GRAMIAN_MFMA_F64 2
#define WG_FLAG_GRAMIAN_MFMA_F32 4

/* Per-gait state carried from tick to tick. */
typedef struct wg_gait_state {
  /* scheduling: ZMPVelocityReferencedQP members + the caller's 5 ms clock */
  double clock;             /* m_InternalClock at which the NEXT tick fires */
  double upper_time_limit;  /* UpperTimeLimitToUpdate_ */
  double time_to_stop;      /* TimeToStopOnLineMode_ */
  int tick_count;
  int running;              /* Running_ */
  int ending_phase;         /* EndingPhase_ (":stoppg") */
  int online;               /* m_OnLineMode */
  /* NewVelRef_.Local */
  double vref[3];
  /* LinearizedInvertedPendulum2D state; com_z = starting CoM height (:303) */
  double com_x[3], com_y[3], com_z;
  /* IntermedData_->SupportState()  (support_state_t, privatepgtypes.hh:291-320) */
  int phase, foot, nb_steps_left, step_number, state_changed, pad0_;
  double time_limit, start_time, sup_x, sup_y, sup_yaw;
  /* SupportFSM rotation bookkeeping (SupportFSM.hh:117-134) */
  int in_translation, in_rotation, nb_steps_after_rotation, rot_support_foot,
      post_rotation_phase, nb_steps_ssds;
  /* OrientationsPreview::TrunkState_ / TrunkStateT_ (yaw only) */
  double trunk_yaw[3], trunkT_yaw[3];
  /* what the tick reads from the four deques: with the reference's cadence
   * (20 samples pushed per tick, one popped per 5 ms call) deque.front() is the
   * previous tick's sample #11, deque[size-2] its #18 and deque.back() its #19 */
  wg_foot_sample_t lf[3], rf[3];          /* [0] front, [1] back-1, [2] back */
  double front_com_x[3], front_com_y[3];  /* FinalCOMTraj_deq[0] */
  /* swing-foot height polynomial, set only when the support state changes
   * (OnLineFootTrajectoryGeneration.cpp:285-286) */
  double poly_z[5];
} wg_gait_state_t;

#define WG_SAMPLES_PER_TICK 20   /* QP_T_ / m_SamplingPeriod */

/* What one tick appends to the four deques + solver diagnostics.  Arrays of it should start on a 128-byte boundary
 * (hipMalloc / wg_host_alloc do). */
typedef struct wg_tick_out {
  double jerk_x, jerk_y;                       /* control applied to the LIPM */
  int ifail, n_iter, nact, n, m, nb_prw_steps; /* QP dimensions: n = 2N+2s, m = 1+4N+5s */
  double com_x[WG_SAMPLES_PER_TICK][3], com_y[WG_SAMPLES_PER_TICK][3];
  double com_yaw[WG_SAMPLES_PER_TICK][2];
  double zmp_x[WG_SAMPLES_PER_TICK], zmp_y[WG_SAMPLES_PER_TICK];
  wg_foot_sample_t lf[WG_SAMPLES_PER_TICK], rf[WG_SAMPLES_PER_TICK];
  /* the newest sample ALREADY in the feet queues before this tick: the double-support branch of
   * interpolate_feet_positions rewrites it (OnLineFootTrajectoryGeneration.cpp:333-336, k = 0) */
  wg_foot_sample_t lf_back, rf_back;
  /* sizeof == 7808 = 61 cache lines of 128 B (ABI 5; it was 7688, 8 B past 60 lines): in an array of these no line is shared
   * by two gaits' structs.  The tick writes zeros here, so the struct's bytes do not depend on what the buffer held.  (The
   * write amplification of an outs-on launch -- 11.3 KB leave the L2 per stored struct -- is the strided 8-byte stores of this
   * array-of-structs layout, not shared lines: DESIGN 2.) */
  double pad_[15];
} wg_tick_out_t;

/* Defaults of every constant the reference hard-codes; robot part = jrl-dynamics' sample robot. */
void wg_model_defaults(wg_model_t *model);

/* State after ZMPVelocityReferencedQP::InitOnLine (:212-319): standing in double
 * support on the left foot, queues holding the 8 start samples. */
void wg_gait_init(const wg_model_t *model, wg_gait_state_t *state,
                  const double com0[3] /* x y z */, const double left_xyt[3],
                  const double right_xyt[3] /* x y theta[deg] */);


/* Upload the model and build, on the device, what the reference builds once per gait in the
 * ZMPVelocityReferencedQP constructor and InitOnLine: the condensed cart-table maps S/U
 * (RigidBodySystem::compute_dyn_cjerk, rigid-body-system.cpp:377-452) and the invariant Hessian block
 * beta*I + alpha*Uv'Uv + gamma*Uz'Uz (GeneratorVelRef::build_invariant_part, generator-vel-ref.cpp:587-614).
 * These tables are constants of the model (a few KiB, 3 x 2N^3 flop once per process); they are formed on
 * the host in the reference's exact summation order -- so that the per-tick QPs are bit-identical to the
 * reference's -- and uploaded once. */
int wg_mpc_configure(const wg_model_t *model);
/* Optional: allocate the tick / run kernels' per-block solver slots and work queue for fleets of up to max_gaits now.  Without
 * it every launch sizes them for its own grid (a one-robot caller pays for one slot, not for a fleet's; growing never frees
 * what a launch in flight may be using). */
int wg_mpc_reserve(int max_gaits);

/* One MPC tick for each of B gaits (replaces B calls of ZMPVelocityReferencedQP::OnLine with
 * time + 1e-5 > UpperTimeLimitToUpdate_, ZMPVelocityReferencedQP.cpp:346-452).
 *   states  B structs, read and written; state->clock must hold the control-loop time of the tick
 *           (`advance_calls` > 0 adds that many control periods to it first, the way
 *           RunOneStepOfTheControlLoop does, PatternGeneratorInterfacePrivate.cpp:1256)
 *   outs    B structs or NULL (NULL: only the state is advanced)
 *   diag    B x 6 ints {ifail, n_iter, nact, n, m, nb_prw_steps} or NULL
 *   hist    B x hist_cap active-set add(+)/drop(-) log or NULL, hist_len B or NULL
 * The kernels keep a few solver arrays per block in a buffer of the context (what does not fit the CU's LDS at the
 * residency they run at), so launches of the tick / run entry points ON ONE CONTEXT do not overlap on the device.  The library
 * sees to that itself: a launch that arrives on a different stream while the context's previous tick / run launch has not
 * completed is enqueued BEHIND it (hipStreamWaitEvent on an event the previous launch left) -- a pipeline that orders its
 * streams with events of its own is accepted as it is, an unordered one is serialised instead of corrupted.  Streams that
 * are meant to overlap take one context each (wg_ctx_create).  With WG_OVERLAP_STRICT=1 in the environment when the context is
 * created (or after wg_set_overlap_strict(1)) such a launch is refused instead (WG_ERR_BUSY, nothing launched): a way to find
 * serialisation that was not intended; wg_overlap_serialised() counts the launches that were ordered.  The ordering test, the
 * launch and the event record are one critical section per context (host threads may share a context).
 * With more gaits than the device keeps resident, a call that follows another one on the same `states` array starts the gaits
 * in the order of decreasing QL iteration count of that previous tick (scheduling only: no result depends on it). */
int wg_mpc_tick_batch(int B, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls,
                      int *hist, int hist_cap, int *hist_len);
int wg_mpc_tick_batch_dev(int B, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls,
                          int *hist, int hist_cap, int *hist_len, void *hip_stream);
/* n_ticks consecutive ticks of every gait in ONE launch (fleet simulation, Monte-Carlo gaits).  A gait's tick t+1
 * depends only on its own tick t, so the batch does not synchronise between ticks: resident waves pull (gait, next
 * tick) items from a device-side queue, and a gait is offered again as soon as its tick is done.  Same results as
 * n_ticks calls of wg_mpc_tick_batch_dev with the same advance_calls, bit for bit; the velocity references stay what they
 * are for the whole launch (change them between launches with wg_mpc_set_velref_dev).
 *   outs  n_ticks x B (tick-major) or NULL;  diag  n_ticks x B x 6 (tick-major) or NULL.
 * No add/drop history in this mode.  The queue lives in a buffer of the context: one such launch in flight per context at
 * a time (launches on one stream are fine -- they run one after the other). */
int wg_mpc_run_batch_dev(int B, wg_gait_state_t *states, int n_ticks, int advance_calls, wg_tick_out_t *outs, int *diag,
                         void *hip_stream);
/* The same with the velocity references staged ahead: before tick t = 0, period, 2 period, ... of the launch, gait g's
 * reference becomes vref_sched[(t / period) * 3 B + 3 g + {0, 1, 2}] (DEVICE pointer, ceil(n_ticks / period) x B x 3
 * doubles) -- exactly what a loop of { wg_mpc_set_velref_dev; wg_mpc_run_batch_dev(period ticks) } does, bit for bit, in one
 * launch: the batch does not drain at every change of the references.  The batched form of a caller that issues
 * ":setVelReference" / setVelocityReference (patterngeneratorinterface.hh:291-293, ZMPVelocityReferencedQP.hh:103-114)
 * every `period` ticks of the control loop.  period >= 1; vref_sched == NULL: wg_mpc_run_batch_dev. */
int wg_mpc_run_sched_dev(int B, wg_gait_state_t *states, int n_ticks, int advance_calls, const double *vref_sched,
                         int period, wg_tick_out_t *outs, int *diag, void *hip_stream);
/* NewVelRef_ <- (vx, vy, vyaw) for every gait (":setVelReference", ZMPVelocityReferencedQP.hh:103-114);
 * vref = B x 3 doubles, DEVICE pointers. */
int wg_mpc_set_velref_dev(int B, wg_gait_state_t *states, const double *vref, void *hip_stream);
/* One robot (BASELINE configs[1]: batch = 1 -- what a drop-in caller of ZMPVelocityReferencedQP::OnLine has, one tick per
 * 0.1 s of walking): the same tick with the caller's state, outputs and diagnostics in HOST-MAPPED memory from
 * wg_host_alloc.  No staging copies and no device synchronisation: the kernel reads the state over the bus, works on a device
 * copy, writes state / out / diag back and releases a completion counter the call spins on.  Same bytes as
 * wg_mpc_tick_batch(1, ...); out and diag may be NULL.  Runs on a stream of the context, ordered behind the context's other
 * tick / run launches like any launch on another stream (above). */
int wg_host_alloc(void **out, size_t bytes);
void wg_host_free(void *p);
int wg_mpc_tick_pinned(wg_gait_state_t *state, wg_tick_out_t *out, int *diag, int advance_calls);
/* The QP of every gait's NEXT tick exactly as QPProblem::solve would hand it to ql0001_ (qp-problem.cpp:245-279), without
 * advancing anything: Q (C), D (d), DU (A, row 0 the dummy row, mmax >= m + 1 rows), DS (b), XL, XU -- the arrays
 * QPProblem::dump_problem prints (qp-problem.cpp:639-653), which the reference writes to /tmp/Problem_<time>.dat when a solve
 * fails (ZMPVelocityReferencedQP.cpp:399-402).  Column-major with the caller's leading dimensions (nmax, mmax), zero-padded;
 * n[g], m[g] receive the sizes (m counts the dummy row, as m_ does).  `advance_calls` as in wg_mpc_tick_batch.  The states are
 * not modified.  Feeding the result to wg_qp_solve_batch gives the x the fused tick computes, bit for bit. */
int wg_mpc_assemble_batch(int B, const wg_gait_state_t *states, int advance_calls, int nmax, int mmax, double *C, double *d,
                          double *A, double *b, double *xl, double *xu, int *n, int *m);
int wg_mpc_assemble_batch_dev(int B, const wg_gait_state_t *states, int advance_calls, int nmax, int mmax, double *C, double *d,
                              double *A, double *b, double *xl, double *xu, int *n, int *m, void *hip_stream);
/* LDS bytes one gait occupies in the tick kernel for the configured model. */
size_t wg_mpc_tick_lds_bytes(void);
/* the same figure for any model, without configuring it (host arithmetic: lets callers and tests reason about
 * residency -- a gfx950 CU has 160 KiB of LDS, handed out in 1280-byte granules); 0 if N is out of range */
size_t wg_mpc_tick_lds_bytes_for(const wg_model_t *model);

/* Kajita preview-control gains (host, no device work) -----------------------
 *
 * wg_riccati_solve replaces
 *     OptimalControllerSolver(A, b, c, Q, R, Nl) + ComputeWeights(mode) + GetK/GetF
 *     src/PreviewControl/OptimalControllerSolver.hh:143-144, OptimalControllerSolver.cpp:97-126, 200-352
 * for a single-input single-output system x+ = A x + b u, p = c x of order n <= 8 (A row-major n x n):
 * P = stabilising solution of the discrete Riccati equation with weights Q (output) and R (input),
 *     K[n]  = (R + b'Pb)^-1 b'PA,
 *     F[Nl] = (R + b'Pb)^-1 b' ((A - bK)')^k  (c'Q            mode WG_RICCATI_WITH_INITIALPOS
 *                                              P c'Q          mode WG_RICCATI_WITHOUT_INITIALPOS).
 * wg_riccati_gains replaces PreviewControl::ComputeOptimalWeights (src/PreviewControl/PreviewControl.cpp:198-322):
 * it builds the cart-table system for sampling period T and CoM height zc (g = 9.81) -- 3 states for
 * WITH_INITIALPOS, the 4-state error system for WITHOUT_INITIALPOS -- and returns
 *     WITHOUT_INITIALPOS: K = {Ks, Kx[0], Kx[1], Kx[2]};  WITH_INITIALPOS: K = {Kx[0] (= Ks), Kx[1], Kx[2], 0}.
 * The reference passes Q = 1, R = 1e-6 (WITHOUT) or 1e-5 (WITH), Nl = (int)(preview time / T).
 * For a fleet with a CoM height per gait, wg_riccati_gains_batch_dev (below, "Fleets with a CoM height per gait") makes the
 * gains of every gait on the device, from the same arithmetic and to the same bits. */
#define WG_RICCATI_WITH_INITIALPOS 0
#define WG_RICCATI_WITHOUT_INITIALPOS 1
int wg_riccati_solve(int n, const double *A, const double *b, const double *c, double Q, double R, int Nl, int mode,
                     double *K, double *F);
int wg_riccati_gains(double T, double zc, double Q, double R, int Nl, int mode, double *K, double *F);

/* PLDP: primal active-set solver in LQ-preconditioned coordinates (Dimitrov 2008) with OptCholesky updates ----------
 *
 * wg_pldp_configure replaces the constructor
 *     PLDPSolver(CardU, iPu, Px, Pu, iLQ)            src/Mathematics/PLDPSolver.cpp:40-96 (+ PrecomputeiPuPx :208-285)
 * and wg_pldp_solve_batch replaces, batched over B independent problems, each with its own hot-start state,
 *     PLDPSolver::SolveProblem(CstPartOfTheCostFunction, NbOfConstraints, LinearPartOfConstraints,
 *                              CstPartOfConstraints, ZMPRef, XkYk, X, SimilarConstraint,
 *                              NumberOfRemovedConstraints, StartingSequence)      PLDPSolver.cpp:654-1007
 * including the row-append Cholesky of E E' it drives,
 *     OptCholesky::AddActiveConstraint / UpdateCholeskyMatrixFortran              OptCholesky.cpp:92-104, 171-223
 * called from ZMPConstrainedQPFastFormulation::BuildZMPTrajectoryFromFootTrajectory
 *     src/ZMPRefTrajectoryGeneration/ZMPConstrainedQPFastFormulation.cpp:1318-1327.
 *
 *     minimise 1/2 |v|^2 + D'v   s.t.  A v + b >= 0,      v in R^(2N)  (x block, then y block)
 *
 *   N        preview length (CardU), 1 <= N <= WG_PLDP_N;  iPu, Pu: N x N row-major, Px: N x 3 row-major
 *   mcap     slot size of the per-problem arrays, m[b] <= mcap <= WG_PLDP_MMAX
 *   m        B          number of constraint rows of problem b
 *   D        B x 2N     linear part of the cost
 *   A        B slots of (mcap+1)*2N doubles; problem b is COLUMN-major with LEADING DIMENSION m[b]+1, exactly as
 *                       BuildConstraintMatrices writes DPu (ZMPConstrainedQPFastFormulation.cpp:773-775, 893-905)
 *   b        B x mcap   constant part (DPx)
 *   zmpref   B x 2N,  xkyk B x 6 (x, dx, ddx, y, dy, ddy)
 *   similar  B x mcap   SimilarConstraint: 0, or the (negative) offset to an earlier row with A_i = -A_j
 *                       (FootConstraintsAsLinearSystem.cpp:55-93); positive offsets are rejected
 *   n_removed, starting   B each: NumberOfRemovedConstraints, StartingSequence
 *   max_iter  the reference stops on a 1.3 ms wall-clock budget (PLDPSolver.cpp:51-52, 889-900), which cannot be
 *             reproduced; max_iter <= 0 runs to completion (the reference when the budget is not hit), otherwise the
 *             loop ends after max_iter iterations, like a budget that expires during that iteration
 *   states   B          hot-start state, read and updated (m_PreviouslyActivatedConstraints, m_PreviousZMPSolution)
 *   X        B x 2N     solution;   ret B: 0, WG_PLDP_NAN (reference returns -1), WG_PLDP_NEG_ALPHA (reference calls
 *                       exit(0)), WG_PLDP_CAPACITY (more than WG_PLDP_ACTIVE_CAP active rows; E E' is singular long
 *                       before that; or a hot-start row prev_active[i] - n_removed[b] >= m[b], which the reference would
 *                       index its constraint matrix with: refused like a full factor), WG_PLDP_BAD_INPUT (a positive or
 *                       out-of-range SimilarConstraint offset).  A hot start refused with WG_PLDP_CAPACITY solves nothing:
 *                       n_iter = 0, X is the initial solution (ComputeInitialSolution on the state as it came in), the
 *                       state's n_prev is cleared, its prev_zmp and internal_time stay as they were
 *                       (WG_PLDP_NAN: a non-finite X[0] or X[N]; the state's members and prev_zmp are stored as the
 *                       reference stores them before it tests, internal_time does not advance)
 *   n_iter   B          m_ItNb;  active B x mcap / n_active B: m_ActivatedConstraints in activation order (or NULL) */
#define WG_PLDP_N 16
#define WG_PLDP_MMAX (8 * WG_PLDP_N)
/* rows the packed Cholesky factor L of E E' holds.  With 2N = 32 unknowns E E' is singular beyond 32 active rows (at most two
 * faces of a ZMP polygon meet per instant), so 40 is margin, not a limit of the method -- and L is what decides how many problems
 * a CU holds (64 rows: 21 KB of LDS per problem, 7 per CU; 40: 10.9 KB, 14 per CU: +36 % solves/s).  The Dimitrov tick kernel
 * uses the same cap. */
#define WG_PLDP_ACTIVE_CAP 40
#define WG_PLDP_NAN (-1)
#define WG_PLDP_NEG_ALPHA (-2)
#define WG_PLDP_CAPACITY (-3)
#define WG_PLDP_BAD_INPUT (-4)
typedef struct wg_pldp_state {
  int n_prev;
  int prev_active[WG_PLDP_MMAX];
  int pad_;
  double prev_zmp[2 * WG_PLDP_N];
  double internal_time;
} wg_pldp_state_t;
int wg_pldp_configure(int N, const double *iPu, const double *Px, const double *Pu);
int wg_pldp_solve_batch(int B, int mcap, const int *m, const double *D, const double *A, const double *b,
                        const double *zmpref, const double *xkyk, const int *similar, const int *n_removed,
                        const int *starting, int max_iter, wg_pldp_state_t *states, double *X, int *ret, int *n_iter,
                        int *active, int *n_active);
/* same, DEVICE pointers, asynchronous on hip_stream */
int wg_pldp_solve_batch_dev(int B, int mcap, const int *m, const double *D, const double *A, const double *b,
                            const double *zmpref, const double *xkyk, const int *similar, const int *n_removed,
                            const int *starting, int max_iter, wg_pldp_state_t *states, double *X, int *ret,
                            int *n_iter, int *active, int *n_active, void *hip_stream);
/* LDS bytes one problem occupies in the PLDP kernel. */
size_t wg_pldp_lds_bytes(void);

/* Dimitrov-2008 receding-horizon tick around PLDP, batched over independent gaits ------------------------------------
 *
 * wg_dimitrov_configure replaces ZMPConstrainedQPFastFormulation::InitConstants
 *     src/ZMPRefTrajectoryGeneration/ZMPConstrainedQPFastFormulation.cpp:692-703  (= InitializeMatrixPbConstants :158-246,
 *     BuildingConstantPartOfTheObjectiveFunction[QLDANDLQ] :384-560, BuildingConstantPartOfConstraintMatrices :597-690)
 * in mode PLDP (:55) and hands the resulting iPu, Px, Pu to the PLDP back-end (the PLDPSolver constructor, :104-109).
 * wg_dimitrov_tick_batch replaces one pass of the loop body of BuildZMPTrajectoryFromFootTrajectory (:1180-1400):
 *     BuildConstraintMatrices (:759-1022)  from the ZMP polytopes of the N previewed instants
 *     D = OptB xk - OptC ZMPRef (:1254-1262), PLDPSolver::SolveProblem (:1322-1339), X <- iLQ' X (:1355-1381),
 *     LinearizedInvertedPendulum2D::Interpolation + OneIteration (:1388-1392).
 * The polytopes are what FootConstraintsAsLinearSystem::BuildLinearConstraintInequalities produces
 * (LinearConstraintInequality_t, pgtypes.hh:158-165): rows A_j (2 coefficients), B_j, the centre (the ZMP reference)
 * and SimilarConstraints; constraint sense A_j . zmp + B_j >= 0.  The caller supplies, per gait, the polytope of each
 * previewed instant (N entries) -- 2 KB per gait-tick instead of the 33 KB dense DPu. */
#define WG_POLY_MAX_ROWS 8            /* "8 constraints per support foot", :771-772 */
/* the QP back-end of the tick, m_FastFormulationMode (ZMPConstrainedQPFastFormulation.hh:263-265; the constructor takes PLDP, :55) */
#define WG_DIMITROV_PLDP 0            /* PLDPSolver on the LQ-preconditioned problem (v = LQ u, Hessian = I), X <- iLQ' X            */
#define WG_DIMITROV_QLD 1             /* "QLD" (:1297-1320): ql0001_ on the problem as it stands -- Q = OptA (:382-389), constraint  */
                                      /* matrix from the triangular Pu' (:891-904), cost vector from OptB / OptC as built (:545-556), */
                                      /* iwar[0] = 1, eps = 1e-8, bounds +-1e8 (:1280-1292); X is the jerk itself (:1383).  With the   */
                                      /* reference's own OptA (alpha VPu' instead of alpha VPu'VPu, :524-527: not symmetric, its upper  */
                                      /* triangle not positive definite) ql0001_ answers ifail = 2 on the first tick -- here as there. */
#define WG_DIMITROV_QLDANDLQ 2        /* "QLDANDLQ": ql0001_ on the SAME preconditioned problem PLDP gets -- Q = I handed over as its   */
                                      /* own Cholesky factor (iwar[0] = 0, :1288-1289), DPu from iLQ Pu' (:905-918), X <- iLQ' X        */
typedef struct wg_dimitrov_model {
  int N, solver;                      /* m_QP_N = 16 (:83); WG_DIMITROV_PLDP (0, the reference's default), _QLD or _QLDANDLQ */
  double T;                           /* m_QP_T = 0.1                                 :82  */
  double Tctrl;                       /* m_SamplingPeriod = 0.005 */
  double com_height;                  /* m_ComHeight = 0.80                           :87  */
  double alpha, beta;                 /* 200, 1000                                    :95-96 */
} wg_dimitrov_model_t;
typedef struct wg_zmp_polytope {
  int nrows, pad_;
  int similar[WG_POLY_MAX_ROWS];
  double A[WG_POLY_MAX_ROWS][2];
  double B[WG_POLY_MAX_ROWS];
  double centre[2];
} wg_zmp_polytope_t;
typedef struct wg_dimitrov_state {
  double xk[6];                       /* LIPM state x, dx, ddx, y, dy, ddy  (m_2DLIPM->GetState) */
  wg_pldp_state_t pldp;               /* the solver's hot-start members */
  int n_removed;                      /* NumberOfRemovedConstraints for the next solve (:1340) */
  int starting;                       /* StartingSequence: 1 before the first tick (:1167, :1339) */
} wg_dimitrov_state_t;
typedef struct wg_dimitrov_out {
  double jerk_x, jerk_y;              /* ptX[0], ptX[N] */
  int ret, n_iter, n_active, m;       /* PLDP return code (see wg_pldp_solve_batch), m_ItNb, active rows, rows;
                                       * WG_DIMITROV_QLD: ql0001_'s ifail (0 = solved), its iteration count, active constraints, rows */
  /* what Interpolation writes for lk = 0..interval (21 samples; the last one is overwritten by the next tick) */
  double com_x[WG_SAMPLES_PER_TICK + 1][3], com_y[WG_SAMPLES_PER_TICK + 1][3];
  double zmp_x[WG_SAMPLES_PER_TICK + 1], zmp_y[WG_SAMPLES_PER_TICK + 1];
  double X[2 * WG_PLDP_N];            /* ptX: the jerks over the horizon (x block, then y block), un-preconditioned (:1355-1383) */
} wg_dimitrov_out_t;
void wg_dimitrov_defaults(wg_dimitrov_model_t *model);
int wg_dimitrov_configure(const wg_dimitrov_model_t *model);
/* the constants InitConstants leaves behind, for inspection: iLQ, OptC 2N x 2N, OptB 2N x 6, Pu (= iLQ Pu'), iPu N x N,
 * Px N x 3, all row-major; any pointer may be NULL */
int wg_dimitrov_get_constants(double *iLQ, double *OptB, double *OptC, double *Pu, double *iPu, double *Px);
/* what mode QLD works with: Q = m_Q (2N x 2N, ql0001_'s column-major layout, :382-389), OptB (2N x 6) and OptC (2N x 2N) as
 * BuildingConstantPartOfTheObjectiveFunction leaves them before the LQ step (:545-556), PuT = Pu' (N x N, [k N + i], :629-637);
 * row-major unless said otherwise; any pointer may be NULL */
int wg_dimitrov_get_qld_constants(double *Q, double *OptB, double *OptC, double *PuT);
/* polys: B x N polytopes (instant-major per gait); outs may be NULL.  A gait whose solve returns ret != 0 keeps its
 * state (xk not advanced), like the reference which stops there (:1343-1347).  With model.solver == WG_DIMITROV_QLD / _QLDANDLQ the
 * solve is the in-wave ql0002 of wg_qp_solve_batch -- the back-ends of this tick whose CPU counterpart is the reference's own
 * compiled qld.cpp; the PLDP hot-start members of the state are carried along untouched, max_iter is ignored.  With more gaits
 * than resident waves they start longest-solve-first by the previous tick on the same state array (scheduling only). */
int wg_dimitrov_tick_batch(int B, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs,
                           int max_iter);
int wg_dimitrov_tick_batch_dev(int B, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states,
                               wg_dimitrov_out_t *outs, int max_iter, void *hip_stream);

/* Kajita stage-1 preview control, batched over independent gaits ------------------------------------------------------
 *
 * wg_preview_configure replaces the members PreviewControl holds once ComputeOptimalWeights
 * (src/PreviewControl/PreviewControl.cpp:198-322) or ReadPrecomputedFile (:134-194) has run: sampling period T and CoM
 * height zc (=> m_A, m_B, m_C :203-214), m_Kx, m_Ks and the window gains m_F[nl], nl = (int)(preview time / T).
 * (wg_riccati_gains computes them; mode WITHOUT_INITIALPOS returns K = {Ks, Kx[0..2]}.)
 * wg_preview_run_batch replaces, for each of B independent gaits, L consecutive calls
 *     PreviewControl::OneIterationOfPreview(x, y, sxzmp, syzmp, ZMPPositions, lindex = l, zmpx2, zmpy2, Simulation)
 *     src/PreviewControl/PreviewControl.cpp:324-374        (OneIterationOfPreview1D :376-420 is one axis of it)
 * for l = 0..L-1 on a ZMP reference queue of L + nl - 1 samples (the reference throws when fewer than nl samples are
 * left, :341-344; here the caller sizes the queue).  Same operation order as the reference, bit for bit.
 *   zmp_x, zmp_y   B x (L + nl - 1)   ZMPPositions[.].px / .py per gait
 *   state          B x 8              x(0..2,0), y(0..2,0), sxzmp, syzmp -- read, advanced L steps, written back
 *   com            B x L x 6          x and y after each step (what callers push on the CoM buffer), may be NULL
 *   zmp2           B x L x 2          zmpx2, zmpy2 of each step, may be NULL
 *   simulation     the reference's `Simulation` flag: accumulate the ZMP tracking error into sxzmp / syzmp
 * The _dev variant takes TIME-MAJOR device arrays so that a wave's window reads are contiguous:
 *   zmp_*_tm [(L + nl - 1)][B],  com_tm [L][6][B],  zmp2_tm [L][2][B];  state stays [B][8]. */
#define WG_PREVIEW_NL_MAX 4096
typedef struct wg_preview_gains {
  double T, zc;                       /* m_SamplingPeriod, m_Zc */
  double Ks, Kx[3];                   /* m_Ks, m_Kx */
  int nl, pad_;                       /* m_SizeOfPreviewWindow */
} wg_preview_gains_t;
int wg_preview_configure(const wg_preview_gains_t *gains, const double *F);
int wg_preview_window(void);          /* nl of the configured gains, 0 before wg_preview_configure */
int wg_preview_run_batch(int B, int L, const double *zmp_x, const double *zmp_y, double *state, double *com, double *zmp2,
                         int simulation);
int wg_preview_run_batch_dev(int B, int L, const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm,
                             double *zmp2_tm, int simulation, void *hip_stream);

/* Kajita stage-1 inputs: ZMP reference queue and feet trajectories of a step sequence, batched over gaits ------------
 *
 * wg_zmpdisc_batch replaces, for each of B independent gaits,
 *     ZMPDiscretization::GetZMPDiscretization                  src/ZMPRefTrajectoryGeneration/ZMPDiscretization.cpp:143-173
 * = InitOnLine (:319-513: rest phase of 2 preview windows, then OnLineAddFoot (:573-1020) for every step after the
 * first) + EndPhaseOfTheWalking (:1129-1300), i.e. what PatternGeneratorInterfacePrivate::CreateZMPReferences
 * (PatternGeneratorInterfacePrivate.cpp:1870-1882) obtains for ":stepseq" in Kajita mode -- with
 *     FilterOutValues (:1045-1109) on the window of InitializeFilter (:240-262),
 *     UpdateCurrentSupportFootPosition (:515-558),
 *     FootTrajectoryGenerationStandard::UpdateFootPosition / SetParameters
 *         src/FootTrajectoryGeneration/FootTrajectoryGenerationStandard.cpp:411-566, 150-186,
 *     Polynome::Compute, Polynome3/4/5::SetParameters   src/Mathematics/Polynome.cpp:44-53, PolynomeFoot.cpp:41-57, 100-120, 174-195.
 * The steps are RelativeFootPosition records (pgtypes.hh:100-108) as StepStackHandler::ReadStepSequenceAccordingToWalkMode
 * (StepStackHandler.cpp:128-175) leaves them: theta in DEGREES, SStime / DStime = the configured support times,
 * stepType 1.  Output per gait: L = wg_zmpdisc_length(model, steps, n_steps) samples at period T of
 *     the filtered ZMP reference (px, py) -- the queue PreviewControl::OneIterationOfPreview reads,
 *     its heading theta and stepType, and both feet (x, y, z, theta, omega, omega2, stepType).
 *   steps      B x smax  (gait b uses the first n_steps[b]; 2 <= n_steps[b] <= smax <= WG_ZMPDISC_MAX_STEPS)
 *   init_feet  B x 6     left x, y, theta, right x, y, theta at the start (EvaluateStartingState's outputs)
 *   lcap       row length of the per-gait output arrays (>= every gait's L; samples past L are left untouched)
 *   zmp        B x lcap x 2  (px, py);  zmp_theta B x lcap;  zmp_type B x lcap   (may be NULL each)
 *   left, right  B x lcap x 6;  left_type, right_type  B x lcap                      (may be NULL each)
 *   length     B         L of each gait, or a negative code: WG_ZMPDISC_BAD_INPUT (n_steps out of range, a phase that
 *                        does not fit its own sample count -- the reference would write out of bounds), WG_ZMPDISC_CAPACITY
 * The _dev variant takes device pointers and writes the ZMP queue TIME-MAJOR, zmp_x_tm / zmp_y_tm [lcap][B], exactly
 * what wg_preview_run_batch_dev reads, so that step sequences go to CoM trajectories without leaving the device; samples
 * past a gait's L repeat its last value there (a gait at rest), so that one preview launch can cover a ragged batch. */
#define WG_ZMPDISC_MAX_STEPS 64
#define WG_ZMPDISC_BAD_INPUT (-1)
#define WG_ZMPDISC_CAPACITY (-2)
typedef struct wg_zmpdisc_model {
  double T;                           /* m_SamplingPeriod  0.005 */
  double preview_time;                /* m_PreviewControlTime  1.6 */
  double t_single, t_double;          /* m_Tsingle, m_Tdble  (":singlesupporttime", ":doublesupporttime") */
  double step_height;                 /* m_StepHeight  (":stepheight") */
  double omega;                       /* m_Omega, degrees  (":omega") */
  double modulation;                  /* m_ModulationSupportCoefficient = 0.9   ZMPDiscretization.cpp:99 */
  double zmp_neutral[2];              /* m_ZMPNeutralPosition = 0, 0            :107-108 */
  double zmp_shift[4];                /* m_ZMPShift (step types 3, 4, 5)        :103-105, 693-718 */
  double foot_b, foot_h, foot_f;      /* m_FootB, m_FootH, m_FootF  FootTrajectoryGenerationStandard.cpp:68-71 */
} wg_zmpdisc_model_t;
typedef struct wg_rel_step {
  double sx, sy, theta;               /* RelativeFootPosition, theta in degrees */
  double ss_time, ds_time;            /* SStime, DStime (ds_time == 0 => the model's times, :608-612) */
  int step_type, pad_;
} wg_rel_step_t;
void wg_zmpdisc_defaults(wg_zmpdisc_model_t *model);
/* number of samples GetZMPDiscretization produces for this sequence (host arithmetic), or a negative code */
int wg_zmpdisc_length(const wg_zmpdisc_model_t *model, const wg_rel_step_t *steps, int n_steps);
int wg_zmpdisc_batch(const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                     const double *init_feet, int lcap, double *zmp, double *zmp_theta, int *zmp_type, double *left,
                     int *left_type, double *right, int *right_type, int *length);
int wg_zmpdisc_batch_dev(const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps,
                         const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm,
                         int *length, void *hip_stream);
/* every output on the device, all time-major: zmp_theta_tm / types [lcap][B], left_tm / right_tm [lcap][6][B]
 * (x, y, z, theta, omega, omega2); any output pointer may be NULL */
int wg_zmpdisc_full_batch_dev(const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps,
                              const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm,
                              double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm,
                              int *right_type_tm, int *length, void *hip_stream);

/* The same walk on line: steps as they arrive --------------------------------------------------------------------------
 *
 * The reference's on-line use of ZMPDiscretization -- InitOnLine (:319-513), OnLineAddFoot (:573-1020) per step,
 * EndPhaseOfTheWalking (:1129-1300) -- for B gaits whose steps are decided while they walk.  wg_zmpdisc_begin_dev runs
 * InitOnLine on the first n_steps[b] >= 2 steps and writes samples [0, length[b]); every wg_zmpdisc_append_dev runs
 * OnLineAddFoot on n_steps[b] >= 0 further steps and writes from the gait's sample count on; wg_zmpdisc_end_dev runs
 * EndPhaseOfTheWalking.  The walk only pushes samples, and its filter reads back into samples already filtered, so a sample
 * once written is final and begin, any appends, end leave every output byte wg_zmpdisc_full_batch_dev leaves for the
 * concatenated sequence.  Cost: each step is walked once, however the calls are cut.
 *   state      B        one wg_zmpdisc_state_t per gait, device memory, written by begin (no need to clear it for begin;
 *                       append / end on a blob that begin never wrote is only recognised if the memory was zeroed)
 *   steps      B x smax the steps of THIS call (begin: the walk's first ones; append: the further ones, from index 0),
 *                       gait b uses the first n_steps[b] <= smax; append: 1 <= smax <= WG_ZMPDISC_MAX_STEPS, and
 *                       n_steps[b] == 0 means the gait sits the call out: none of its bytes, length[b] included, is touched
 *   outputs    the layouts of wg_zmpdisc_full_batch_dev (time-major, row stride B), any of them NULL, zmp_x_tm and zmp_y_tm
 *              together; pass the same set to every call of a walk.  With the queue present the filter's look-back is read
 *              from the gait's own rows of it (the reference's deque); without, from the tail kept in the state.
 *   lcap       rows the outputs hold; may grow from call to call (wg_zmpdisc_length_after sizes it)
 *   length     B, may be NULL: samples of the gait after the call, or a negative code
 *   select     wg_zmpdisc_end_dev only, B or NULL: gaits with select[b] == 0 sit the call out untouched and walk on; NULL ends
 *              every gait.  After its end phase a gait's queue rows [length[b], lcap) repeat its last value, the rule of
 *              wg_zmpdisc_batch_dev.
 * Errors are per gait and sticky: WG_ZMPDISC_BAD_INPUT (n_steps out of range, a phase that does not fit its own sample count,
 * append or end on a gait that has ended or never began) or WG_ZMPDISC_CAPACITY (the call's samples do not fit lcap) is
 * decided before the call's first sample; the call then writes nothing for the gait but the code, to length[b] and to the
 * state, where every later call finds it and reports it again.  A neighbour never notices.  A walk has no bound on its
 * number of steps, only zd_length's 2^24 samples.  All three are asynchronous on hip_stream and keep nothing in the context.
 * These entry points were added without a change of wg_abi_version() (no existing signature changed): a caller that must
 * run against older libraries detects them by symbol (dlsym) or, at compile time, by WG_ZMPDISC_STATE_BYTES. */
#define WG_ZMPDISC_TAIL_MAX 52        /* most filter taps a model may have (T >= 1 ms) */
typedef struct wg_zmpdisc_state {
  double support[6];                  /* m_CurrentSupportFootPosition rows 0, 1 */
  double prev_support[2];             /* translation of m_PrevCurrentSupportFootPosition */
  double prev_rel[2];                 /* m_vdiffsupppre */
  double ang_support, ang_zmp;        /* m_AngleDiffToSupportFootTheta, m_AngleDiffFromZMPThetaToSupportFootTheta */
  double left[6], right[6];           /* back() of the feet queues: x, y, z, theta, omega, omega2 */
  double zmp_last[3];                 /* FinalZMPPositions.back(): px, py, theta */
  double zmp_first[2];                /* FinalZMPPositions[0] */
  wg_rel_step_t last_step;            /* m_RelativeFootPositions.front(): the step given last */
  double tail[WG_ZMPDISC_TAIL_MAX][2];/* the last filtered samples, newest first; kept only while the queue outputs are NULL */
  int left_type, right_type;          /* stepType of the feet above */
  int n_samples;                      /* samples written: the walk's clock, in periods T */
  int n_steps;                        /* steps given */
  int ended;                          /* EndPhaseOfTheWalking has run */
  int error;                          /* 0 or the sticky code */
  int begun, pad_;                    /* set by wg_zmpdisc_begin_dev */
} wg_zmpdisc_state_t;
#define WG_ZMPDISC_STATE_BYTES 1144
#ifdef __cplusplus
static_assert(sizeof(wg_zmpdisc_state_t) == WG_ZMPDISC_STATE_BYTES, "wg_zmpdisc_state_t is part of the ABI");
#else
_Static_assert(sizeof(wg_zmpdisc_state_t) == WG_ZMPDISC_STATE_BYTES, "wg_zmpdisc_state_t is part of the ABI");
#endif
/* samples of a walk after the first n_steps >= 2 steps of a sequence, and after its end phase if `ended`: the prefix sums
 * of wg_zmpdisc_length (host arithmetic; ended != 0 and n_steps <= WG_ZMPDISC_MAX_STEPS: wg_zmpdisc_length itself), or a
 * negative code */
int wg_zmpdisc_length_after(const wg_zmpdisc_model_t *model, const wg_rel_step_t *steps, int n_steps, int ended);
int wg_zmpdisc_begin_dev(const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                         const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm,
                         int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm,
                         wg_zmpdisc_state_t *state, int *length, void *hip_stream);
int wg_zmpdisc_append_dev(const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                          int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm,
                          double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm,
                          wg_zmpdisc_state_t *state, int *length, void *hip_stream);
int wg_zmpdisc_end_dev(const wg_zmpdisc_model_t *model, int B, const int *select, int lcap, double *zmp_x_tm,
                       double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm,
                       double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream);

/* The same walks with a model per gait -----------------------------------------------------------------------------------
 *
 * Robots of different size differ in their support times, step height, foot geometry and ZMP offsets, not only in the CoM
 * height the consumers' fleet forms take per gait.  wg_zmpdisc_full_fleet_dev, wg_zmpdisc_begin_fleet_dev, _append_fleet_dev and
 * _end_fleet_dev are wg_zmpdisc_full_batch_dev, _begin_dev, _append_dev and _end_dev word for word, with a wg_zmpdisc_fleet_t in
 * place of the one model: gait b walks with models[model_of[b]], or with models[b] where model_of is NULL (then M == B).
 * CONTRACT: every byte the call writes for gait b -- length[b], its state blob, every output row, the at-rest rows past
 * length[b] -- is the byte the one-model call writes for that gait when handed models[model_of[b]]; what that call leaves
 * untouched stays untouched.  Every field but T may differ from gait to gait, preview_time included (it only enters the sample
 * counts; wg_zmpdisc_length and wg_zmpdisc_length_after take the gait's own model when the caller sizes lcap).
 *   base     read on the host: base.T fixes the filter window, which is the launch's shape (LDS); nothing else of it is read
 *   models   M, DEVICE memory;  model_of  B, DEVICE memory, or NULL
 * A gait whose model's T is not base.T bit for bit, or whose model_of[b] lies outside [0, M), is refused with
 * WG_ZMPDISC_BAD_INPUT like every other per-gait refusal: decided before the gait's first sample, written to length[b] alone in
 * the whole-sequence form, sticky in the state in the on-line forms (an earlier sticky code is reported first); a neighbour
 * never notices.  Pass the same models to every call of a walk.
 * Host-side errors (WG_ERR_BAD_ARG, nothing launched): NULL fleet or models, M < 1, model_of == NULL with M != B, a base.T the
 * one-model calls refuse or whose window leaves no room for the wave's models beside it in LDS (more than 50 taps: T of about
 * 1 ms and below), and everything the one-model calls refuse.  The gaits' models are staged once per wave in LDS beside the
 * filter rings (16 doubles per gait).  Asynchronous on hip_stream; nothing is kept in the context.
 * Added without a change of wg_abi_version(): detect by symbol. */
typedef struct wg_zmpdisc_fleet {
  wg_zmpdisc_model_t base;            /* read on the host; base.T fixes the filter window = the launch shape */
  int M, pad_;
  const wg_zmpdisc_model_t *models;   /* [M] device */
  const int *model_of;                /* [B] device, or NULL: M == B and gait b walks with models[b] */
} wg_zmpdisc_fleet_t;
#define WG_ZMPDISC_FLEET_BYTES 152
#ifdef __cplusplus
static_assert(sizeof(wg_zmpdisc_fleet_t) == WG_ZMPDISC_FLEET_BYTES, "wg_zmpdisc_fleet_t is part of the ABI");
#else
_Static_assert(sizeof(wg_zmpdisc_fleet_t) == WG_ZMPDISC_FLEET_BYTES, "wg_zmpdisc_fleet_t is part of the ABI");
#endif
int wg_zmpdisc_full_fleet_dev(const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps,
                              const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm,
                              double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm,
                              int *right_type_tm, int *length, void *hip_stream);
int wg_zmpdisc_begin_fleet_dev(const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps,
                               const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm,
                               double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm,
                               int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream);
int wg_zmpdisc_append_fleet_dev(const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps,
                                const int *n_steps, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm,
                                int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm,
                                wg_zmpdisc_state_t *state, int *length, void *hip_stream);
int wg_zmpdisc_end_fleet_dev(const wg_zmpdisc_fleet_t *fleet, int B, const int *select, int lcap, double *zmp_x_tm,
                             double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm,
                             double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream);

/* Where the steps come from: the step stack on the device ---------------------------------------------------------------
 *
 * The generators of the reference's StepStackHandler for B gaits at once, in the layout wg_zmpdisc_full_batch_dev,
 * wg_zmpdisc_begin_dev and wg_zmpdisc_append_dev read: a fleet whose commands live in device memory (a planner's output, a
 * policy's tensor) goes from a few numbers per gait to its CoM on one stream.  One call turns every gait's command list into
 * the steps of THIS call, written from index 0 of the gait's row, and their count n_steps[b] -- the arguments of the zmpdisc
 * call behind it.  Every step carries step_type 0, pad_ 0 and the call's ss_time, ds_time.
 *   op                    arguments                reference (src/StepStackHandler.cpp)            step                  keep
 *   WG_STEP_NONE                                                                                   none                  unchanged
 *   WG_STEP_SUPPORT_FOOT  foot                     PrepareForSupportFoot :754-764                  (0, foot 0.095, 0)    unchanged
 *   WG_STEP_ARC           a = x, y, arc_deg; foot  CreateArcInStepStack :299-457                   the arc's steps       the foot it ends on
 *   WG_STEP_LAST_SUPPORT                           FinishOnTheLastCorrectSupportFoot :872-882      (0, keep 0.19, 0)     unchanged
 *   WG_STEP_ADD           a = sx, sy, theta        AddStepInTheStack :850-863 (the call's times)   (sx, sy, theta)       unchanged
 *   WG_STEP_ONLINE        a = x, y, theta          AddStandardOnLineStep(true, ..) :791-832        (x, y + keep 0.19, theta)  -keep
 *   WG_STEP_ONLINE_IDLE                            AddStandardOnLineStep(false, ..) :791-832       (0, keep 0.19, 0)     -keep
 * keep is m_KeepLastCorrectSupportFoot (+1 / -1; a fresh stack holds {1, 0, 0, 0}); it is carried by the stack alone, so a
 * command list gives the same steps however it is cut into calls.  Angles are degrees.  An arc of radius R = |(x, y)| turns
 * by arc_deg in steps of 0.15 m along it, plus one shorter step where they do not divide it; its direction is the sign of y,
 * x < 0 walks it backwards.  x = y = 0 and arc_deg = 0 give no step and keep = foot, as in the reference.  The arguments an
 * op does not take are ignored, but a[] must be finite.
 *   cmds     B x ccap   gait b's list is its first n_cmds[b]
 *   stack    B, in/out  keep, the sticky error, n_given (steps given so far, accumulated), pad_
 *   steps    B x smax   bytes of a row past n_steps[b] are untouched
 *   n_cmds[b] == 0      n_steps[b] = 0 and the stack is untouched: the gait sits out the append that follows
 * Refusals are per gait, decided before the gait's first write and sticky in stack[b].error: a refused call sets
 * n_steps[b] = 0 and stack[b].error and writes nothing else of the gait, and every later call finds the code and does the
 * same.  wg_zmpdisc_begin_dev then refuses the gait with its own sticky code (n_steps < 2) and wg_zmpdisc_append_dev lets it
 * sit out; a neighbour never notices.  The first command, in order, that offends decides the code:
 *   WG_STEPS_BAD_INPUT  an unknown op; a foot that is not +1 / -1 where the op takes one; a non-finite a[]; arc_deg < 0 (a
 *                       declared refusal: the reference pushes one step for it that no generator here restates -- the way
 *                       to walk an arc the other way is the sign of y); a radius that overflows; n_cmds[b] outside
 *                       [0, ccap]; a stack whose keep is not +1 / -1 (never initialised)
 *   WG_STEPS_CAPACITY   the commands give more than smax steps (an arc's count is known before its first step)
 * Host-side errors (WG_ERR_BAD_ARG, nothing launched): a NULL array, B < 0, ccap < 1, smax outside
 * [1, WG_ZMPDISC_MAX_STEPS], non-finite ss or ds.  B == 0 is WG_OK.  Asynchronous on hip_stream; keeps nothing in the context.
 * wg_steps_plan is the same arithmetic for one gait on the host (the same bytes; returns WG_OK with the verdict in
 * stack->error and *n_steps, or WG_ERR_BAD_ARG); wg_steps_count is the number of steps a list gives, for sizing buffers
 * together with wg_zmpdisc_length_after -- a walk's length depends only on the count and the times -- or a code
 * (WG_STEPS_CAPACITY: more than WG_ZMPDISC_MAX_STEPS, what no call can hold).
 * Added without a change of wg_abi_version(): detect by symbol. */
enum { WG_STEP_NONE = 0, WG_STEP_SUPPORT_FOOT, WG_STEP_ARC, WG_STEP_LAST_SUPPORT, WG_STEP_ADD, WG_STEP_ONLINE, WG_STEP_ONLINE_IDLE };
typedef struct wg_step_cmd {
  int op, foot;                       /* foot = +1 / -1 where the op takes one */
  double a[3];
} wg_step_cmd_t;
typedef struct wg_step_stack {
  int keep;                           /* m_KeepLastCorrectSupportFoot (starts at 1) */
  int error;                          /* 0 or the sticky code */
  int n_given, pad_;                  /* steps given so far */
} wg_step_stack_t;
#define WG_STEPS_BAD_INPUT (-1)
#define WG_STEPS_CAPACITY (-2)
int wg_steps_count(const wg_step_cmd_t *cmds, int n_cmds);
int wg_steps_plan(const wg_step_cmd_t *cmds, int n_cmds, double ss, double ds, wg_step_stack_t *stack, int smax,
                  wg_rel_step_t *steps, int *n_steps);
int wg_steps_plan_dev(int B, int ccap, const wg_step_cmd_t *cmds, const int *n_cmds, double ss, double ds,
                      wg_step_stack_t *stack, int smax, wg_rel_step_t *steps, int *n_steps, void *hip_stream);
/* The same with support times per gait (robots of different cadence in one launch): ss, ds are DEVICE arrays of B, and gait b's
 * bytes are those of wg_steps_plan_dev called with ss[b], ds[b].  A gait that runs (no sticky error, n_cmds[b] != 0) with a
 * non-finite ss[b] or ds[b] is refused with WG_STEPS_BAD_INPUT ahead of its commands' own verdict, with the refusal semantics
 * above (n_steps[b] = 0, sticky in stack[b].error, nothing else written); a gait that sits out is not looked at.  Host-side
 * errors as above, the times aside: NULL ss or ds.  Added without a change of wg_abi_version(): detect by symbol. */
int wg_steps_plan_fleet_dev(int B, int ccap, const wg_step_cmd_t *cmds, const int *n_cmds, const double *ss, const double *ds,
                            wg_step_stack_t *stack, int smax, wg_rel_step_t *steps, int *n_steps, void *hip_stream);

/* The preview that follows such a walk: every gait advances over exactly the rows its own queue has made safe -------------
 *
 * wg_preview_follow_dev is wg_preview_run_batch_dev with a range per gait, driven by the `length` array the wg_zmpdisc
 * on-line calls leave on the device: the host does no arithmetic on lengths and reads nothing back, whatever the gaits'
 * step counts and support times are, and whenever each of them begins, is fed or ends.  All pointers are DEVICE pointers,
 * the layouts are those of wg_preview_run_batch_dev with ABSOLUTE rows:
 *   zmp_*_tm [lcap][B]                 the gait's queue from sample 0 (the convention of the wg_zmpdisc on-line calls)
 *   com_tm   [lcap - nl + 1][6][B],  zmp2_tm [lcap - nl + 1][2][B]    may be NULL each; step l of gait b goes to row l
 *   state    [B][8]
 *   length   B         samples gait b holds
 *   done     B, in/out steps gait b has behind it; done[b] == 0 starts a walk from whatever state[b] holds
 * With nl the configured window, safe[b] = max(0, length[b] - nl + 1) are the steps whose window [l, l + nl) lies inside the
 * samples the gait holds -- a sample once written is final, so these steps are final whether or not the gait has ended, and
 * this is where the reference stops as well (PreviewControl.cpp:341-344).  The call runs steps [done[b], safe[b]) from state[b],
 * writes state[b] back and sets done[b] = safe[b]; a resumed gait refills its window from rows [done[b], done[b] + nl) of its
 * own queue.
 *   done[b] == safe[b]                  the gait sits the call out: none of its bytes is touched.
 *   length[b] < 0 (a gait wg_zmpdisc_* refused) or done[b] < 0    the gait sits out as well: errors are sticky through done[b] < 0.
 *   length[b] > lcap or done[b] > safe[b]    refused: done[b] = WG_ERR_BAD_ARG and nothing else of the gait is written.
 * A neighbour never notices a refused or sitting-out gait.  Nothing at or past row length[b] of a gait is read: those rows are
 * unwritten memory while the gait walks.
 * CONTRACT: after any sequence of follow calls interleaved with calls that grow `length`, state[b] and rows [0, done[b]) of
 * com_tm and zmp2_tm are byte for byte what ONE wg_preview_run_batch_dev with L = done[b] over the gait's final queue leaves,
 * however the growth was cut; rows >= done[b] are untouched.  (Running an ended gait past length - nl + 1 -- the at-rest rows
 * of the batch pipeline -- stays with the batch call.)
 * Host-side errors (WG_ERR_BAD_ARG, nothing launched): no wg_preview_configure, B < 0, lcap < nl, a NULL length, done, queue or
 * state.  B == 0 is WG_OK.  Asynchronous on hip_stream; keeps nothing in the context.
 * Cost: both axes of a gait run in one wave, which reads done[b] before its step loop and stores it behind it, four gaits (windows
 * of 64 .. 384 samples) or 32 gaits (other windows) to the wave; a wave takes as long as its longest gait, so an evenly fed
 * fleet loses nothing against the batch call and a lone long gait costs its wave.
 * Added without a change of wg_abi_version(): detect by symbol. */
int wg_preview_follow_dev(int B, int lcap, const int *length, int *done, const double *zmp_x_tm, const double *zmp_y_tm,
                          double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream);

/* Fleets with a CoM height per gait: gains made on the device, preview with gains per gait ---------------------------------
 *
 * A context holds ONE set of gains (wg_preview_configure).  A fleet whose gaits differ in CoM height -- robots of different
 * size, a load sweep, the reference's :comheight per robot -- has a set per gait; these calls make the B sets on the device
 * and walk the fleet with them in one launch.  T, nl, Q and R stay fleet-wide: the window length fixes the kernel's shape.
 *
 * wg_riccati_gains_batch_dev runs wg_riccati_gains(T, zc[b], Q, R, Nl, mode, ...) for every gait b, one lane per gait, from the
 * text the host call is compiled from (csrc/wg_riccati_math.hpp): K, F and the code are the host call's, bit for bit.
 * All pointers are DEVICE pointers:
 *   zc      [B]        CoM heights
 *   K_tm    [4][B]     entry i of gait b at i*B + b; the four numbers wg_riccati_gains returns in K, in its layout per mode
 *                      (WITHOUT_INITIALPOS: Ks, Kx[0], Kx[1], Kx[2] -- what wg_preview_fleet_t takes as it stands)
 *   F_tm    [Nl][B]    time-major, what the fleet preview calls below read; may be NULL when Nl == 0
 *   status  [B]        what the host call returns for the gait: WG_OK, or WG_ERR_BAD_ARG for a height that is not finite or a
 *                      solve that does not converge.  Such a gait gets zeros in its K and F columns (never NaN); its
 *                      neighbours are not touched by it.
 * Host-side errors (WG_ERR_BAD_ARG, before any device call): B < 0, T <= 0, R <= 0, an unknown mode, Nl < 0 or
 * Nl > WG_PREVIEW_NL_MAX, a NULL zc, K_tm, status or (Nl > 0) F_tm.  B == 0 is WG_OK.  Asynchronous on hip_stream; keeps nothing
 * in the context.  wg_riccati_gains_batch is the same with HOST pointers, gait-major (K [B][4], F [B][Nl]), staged through the
 * context's stream like the other host forms; it returns when the results are in place.
 *
 * wg_preview_run_fleet_dev and wg_preview_follow_fleet_dev are wg_preview_run_batch_dev and wg_preview_follow_dev with the
 * gains of `fleet` instead of the context's: array shapes, length / done semantics, sitting out and refusals are those calls'
 * word for word, with nl = fleet->nl.  Gait b runs with A, B of fleet->T, C = [1, 0, -zc[b] / 9.81], Ks = K_tm[b],
 * Kx[i] = K_tm[(i + 1) * B + b] and F[i] = F_tm[i * B + b], and gives byte for byte what a context configured with those
 * gains gives for it.  The arrays of `fleet` are DEVICE arrays, the struct itself is read on the host during the call.
 * They read nothing of the context's configured gains and write nothing to them (no wg_preview_configure is needed).
 * Windows of 64 .. 384 samples run eight lanes per gait and axis, each lane with its own gait's taps in registers; other
 * windows run one lane per gait and axis.
 * Host-side errors (WG_ERR_BAD_ARG, before any device call): a NULL fleet or a NULL array in it, nl < 1 or
 * nl > WG_PREVIEW_NL_MAX, T <= 0, B < 0, L < 0, a NULL queue or state; follow: a NULL length or done, lcap < nl.
 * Added without a change of wg_abi_version(): detect by symbol. */
typedef struct wg_preview_fleet {
  double T;
  int nl, pad_;
  const double *zc;   /* [B]      device */
  const double *K_tm; /* [4][B]   device: Ks, Kx[0], Kx[1], Kx[2] */
  const double *F_tm; /* [nl][B]  device */
} wg_preview_fleet_t;
int wg_riccati_gains_batch_dev(int B, double T, const double *zc, double Q, double R, int Nl, int mode, double *K_tm,
                               double *F_tm, int *status, void *hip_stream);
int wg_riccati_gains_batch(int B, double T, const double *zc, double Q, double R, int Nl, int mode, double *K, double *F,
                           int *status);
int wg_preview_run_fleet_dev(int B, int L, const wg_preview_fleet_t *fleet, const double *zmp_x_tm, const double *zmp_y_tm,
                             double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream);
int wg_preview_follow_fleet_dev(int B, int lcap, const int *length, int *done, const wg_preview_fleet_t *fleet,
                                const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm,
                                double *zmp2_tm, int simulation, void *hip_stream);

/* ZMP polytopes of a feet trajectory ----------------------------------------------------------------------------------
 *
 * wg_foot_constraints replaces FootConstraintsAsLinearSystem::BuildLinearConstraintInequalities
 *     src/Mathematics/FootConstraintsAsLinearSystem.cpp:258-539   (+ ComputeLinearSystem :97-256,
 *     FindSimilarConstraints :55-92, ComputeConvexHull::DoComputeConvexHull src/Mathematics/ConvexHull.cpp:88-203):
 * one polytope per support phase of a 5 ms feet trajectory, A_j . zmp + B_j >= 0, with its validity interval -- the
 * queue ZMPConstrainedQPFastFormulation::BuildConstraintMatrices (:759-1022) walks to fill the wg_zmp_polytope_t of each
 * previewed instant.  Host code, one gait per call (the facade's one robot); a fleet whose feet are on the device builds its
 * queues there with wg_foot_constraints_batch_dev below.
 *   n            samples;  time n;  left, right  n x 6 (x, y, z, theta, omega, omega2);  left_type n (stepType)
 *   sole_w, sole_h   getSoleSize outputs;  constraint_x, constraint_y  the security margins (ConstraintOnX / Y)
 *   polys, t_start, t_end   up to cap entries;  returns the number of polytopes (may exceed cap) or a negative code */
int wg_foot_constraints(int n, const double *time, const double *left, const int *left_type, const double *right,
                        double sole_w, double sole_h, double constraint_x, double constraint_y, int cap,
                        wg_zmp_polytope_t *polys, double *t_start, double *t_end);

/* Dimitrov-2008 fleets without the host between the feet trajectories and the tick -------------------------------------
 *
 * wg_foot_constraints_batch_dev is wg_foot_constraints for B gaits whose feet wg_zmpdisc_full_batch_dev left on the device
 * (FootConstraintsAsLinearSystem.cpp:258-539, :97-256, :55-92, ConvexHull.cpp:88-203): per gait the bytes of the host call
 * wg_foot_constraints(length[b], time, feet of gait b, ..., qcap, ...) -- same state machine, hull, half-plane forms and
 * SimilarConstraints, entries [count, qcap) left untouched.  All pointers are DEVICE pointers.
 *   length       B      samples of each gait as wg_zmpdisc_full_batch_dev wrote them; nothing past length[b] is read
 *   time         lcap   ONE array shared by every gait
 *   left_tm, right_tm  [lcap][6][B],  left_type_tm  [lcap][B]   (the layouts of wg_zmpdisc_full_batch_dev)
 *   queues, t_start, t_end   [B][qcap]
 *   count        B      polytopes of the gait (may exceed qcap, as the host call's return value may), or WG_ERR_BAD_ARG where
 *                       the host call returns it (length[b] < 0 -- a gait wg_zmpdisc_* refused -- or > lcap; a support whose
 *                       corners span no polygon: the queue entries of such a gait are unspecified)
 * The time axis is split across blocks (chunks of wg_foot_constraints_chunk() samples, a kernel constant); the per-chunk
 * counts live in a buffer of the context between the two passes, so launches of one context are ordered like tick launches. */
int wg_foot_constraints_chunk(void);
int wg_foot_constraints_batch_dev(int B, int lcap, const int *length, const double *time, const double *left_tm,
                                  const int *left_type_tm, const double *right_tm, double sole_w, double sole_h,
                                  double constraint_x, double constraint_y, int qcap, wg_zmp_polytope_t *queues,
                                  double *t_start, double *t_end, int *count, void *hip_stream);
/* The same queues on line: grown with the feet trajectories (wg_zmpdisc_begin_dev / _append_dev / _end_dev), each sample
 * classified and each polytope built once.  The reference has no counterpart (InitOnLine / OnLineAddFoot / OnLine /
 * EndPhaseOfTheWalking of ZMPConstrainedQPFastFormulation are empty bodies, ZMPConstrainedQPFastFormulation.cpp:1544-1595): the
 * contract is equality with wg_foot_constraints_batch_dev.  Layouts and arguments are that call's; per gait
 *   done[b]   B, in/out   samples already turned into queue entries by earlier calls.  done[b] == 0 starts a queue: count[b] is
 *                         ignored on input and restarts at 0.  The call consumes samples [done[b], length[b]) and sets
 *                         done[b] = length[b].
 * CONTRACT: after the call, count[b] and the first min(count[b], qcap) entries of queues, t_start, t_end are exactly what
 * wg_foot_constraints_batch_dev writes for length[b] samples; entries [count[b], qcap) are not touched; the last entry's t_end
 * is time[length[b] - 1].  This holds after every call, however the trajectory is cut.  So an entry is final once written,
 * except the last entry's t_end: the next call overwrites that once, with the time of the first new support change or with
 * the new last sample's time (every entry still has exactly one writer per call).  count[b] may exceed qcap as it may in the
 * batch call: positions >= qcap are counted and not stored, and the entry at position qcap - 1 still gets its t_end from the
 * later call that finds the change closing it.
 *   length[b] == done[b]    the gait sits the call out: none of its bytes is touched.
 *   refused, with count[b] = WG_ERR_BAD_ARG, done[b] unchanged and no queue byte written:  length[b] < 0 (a gait
 *       wg_zmpdisc_* refused);  length[b] > lcap;  done[b] < 0;  done[b] > length[b];  done[b] < first_sample;  done[b] > 0
 *       with count[b] < 0 -- errors are sticky through count[b] < 0.  A support whose corners span no polygon gives
 *       WG_ERR_BAD_ARG as in the batch call.  A neighbour never notices.
 *   first_sample   a HOST-side lower bound on every done[b] (0 is always valid): the chunks of the time axis that lie wholly
 *       below it are not launched, so that a long walk does not pay a grid over its past.
 * The feet arrays hold the whole walk from sample 0 (the convention of the wg_zmpdisc on-line calls: lcap / qcap are sized by
 * the caller for the walk; no ring buffer): the support state before a gait's first new sample is read back from them, nothing
 * else is carried from call to call.  Nothing at or past length[b] is read.  Launches are ordered per context exactly like the
 * batch call's (the same buffer of the context).  Added without a change of wg_abi_version(): detect by symbol. */
int wg_foot_constraints_append_dev(int B, int lcap, int first_sample, int *done, const int *length, const double *time,
                                   const double *left_tm, const int *left_type_tm, const double *right_tm, double sole_w,
                                   double sole_h, double constraint_x, double constraint_y, int qcap,
                                   wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream);
/* Both with a sole per gait (robots of different foot size in one launch): soles is a DEVICE array of B in place of the four
 * scalars, everything else is the call above.  Per gait count[b], the queue entries, t_start, t_end and, for the append form,
 * done[b] are those of the one-sole call handed soles[b] -- the half sole minus the margins is made in the gait's lane with the
 * host call's expression -- including the verdict of wg_foot_constraints on a sole it refuses (corners that span no polygon:
 * WG_ERR_BAD_ARG in count[b]), which goes to that gait alone.  Host-side errors as above, and NULL soles.  Launches are
 * ordered per context like the one-sole calls', through the same buffer.  Added without a change of wg_abi_version(): detect by
 * symbol. */
typedef struct wg_sole {
  double sole_w, sole_h;              /* getSoleSize outputs */
  double constraint_x, constraint_y;  /* the security margins (ConstraintOnX / Y) */
} wg_sole_t;
#define WG_SOLE_BYTES 32
#ifdef __cplusplus
static_assert(sizeof(wg_sole_t) == WG_SOLE_BYTES, "wg_sole_t is part of the ABI");
#else
_Static_assert(sizeof(wg_sole_t) == WG_SOLE_BYTES, "wg_sole_t is part of the ABI");
#endif
int wg_foot_constraints_fleet_dev(int B, int lcap, const int *length, const double *time, const double *left_tm,
                                  const int *left_type_tm, const double *right_tm, const wg_sole_t *soles, int qcap,
                                  wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream);
int wg_foot_constraints_append_fleet_dev(int B, int lcap, int first_sample, int *done, const int *length, const double *time,
                                         const double *left_tm, const int *left_type_tm, const double *right_tm,
                                         const wg_sole_t *soles, int qcap, wg_zmp_polytope_t *queues, double *t_start,
                                         double *t_end, int *count, void *hip_stream);

/* Walk audit: how far a ZMP track stays inside its gait's polytope queue -----------------------------------------------
 *
 * The verdict on a walk, on the device: for every control-period sample of every gait the ZMP's margin inside the polytope
 * the gait's queue holds at that time, reduced to one wg_zmp_audit_t per gait.  The rule for "violated" is the reference's own
 * check of the previewed instants, ZMPConstrainedQPFastFormulation::ValidationConstraints (ZMPConstrainedQPFastFormulation.cpp
 * :248-381, called behind `if (0)` at :1403-1414): a constraint row below -1e-8 (:322).  The margin is the geometric one: the
 * least distance to the polytope's boundary lines, positive inside.
 * Per sample k < length[b], with t = time[k] and (x, y) the track's sample:
 *   1. q is the first stored entry with t_start[q] <= t <= t_end[q] (the search of BuildConstraintMatrices, :785-796).  Adjacent
 *      entries share their boundary instant, so the sample at a support change is audited against the EARLIER polytope.  No such
 *      entry, or an entry whose nrows is outside 1 .. WG_POLY_MAX_ROWS: the sample is uncovered.  The queue is taken to be ordered
 *      as the foot-constraints calls write it (t_end non-decreasing, t_start[q] <= t_end[q] <= t_start[q + 1]); the entry found in
 *      a queue that is not is unspecified.
 *   2. for the rows j < nrows:  v_j = (A[j][0] * x + A[j][1] * y) + B[j],  d_j = v_j / sqrt(A[j][0] * A[j][0] + A[j][1] * A[j][1]),
 *      in exactly this order of operations (no contraction; / and sqrt are IEEE on both sides).  A d_j that is not finite counts
 *      as -inf.
 *   3. the sample's margin is the least d_j, the first j on a tie.  An uncovered sample, or one with a non-finite coordinate, has
 *      margin -inf and no row.
 *   4. the sample is violated when it is uncovered, when it is non-finite, or when some v_j < -1e-8 (the raw row value).
 * All of a gait's fields below; margin (margin_tm) optionally receives every sample's margin. */
typedef struct wg_zmp_audit {
  double margin;      /* min over the gait's audited samples of the sample's margin, metres; +inf when none was audited */
  int worst_sample;   /* the FIRST sample that attains it; -1 when none was audited */
  int worst_row;      /* the first row of that sample's polytope that attains it; -1 for a sample without a margin */
  int n_violated;     /* samples that fail the reference's test */
  int n_uncovered;    /* samples whose time lies in no stored queue entry */
  int n_nonfinite;    /* samples with a non-finite coordinate */
  int status;         /* WG_OK, or WG_ERR_BAD_ARG: a refused gait, every other field as the caller left it */
} wg_zmp_audit_t;
#define WG_ZMP_AUDIT_BYTES 32
#ifdef __cplusplus
static_assert(sizeof(wg_zmp_audit_t) == WG_ZMP_AUDIT_BYTES, "wg_zmp_audit_t is part of the ABI");
#else
_Static_assert(sizeof(wg_zmp_audit_t) == WG_ZMP_AUDIT_BYTES, "wg_zmp_audit_t is part of the ABI");
#endif
/* One gait on the host: the bytes of the kernels.  Audits the samples [first_sample, n) of the track px[k * stride], py[k * stride]
 * (HOST pointers) against the first min(count, qcap) entries of polys / t_start / t_end.  first_sample == 0 starts the audit;
 * first_sample > 0 folds the samples into *audit as an earlier call left it (the result is that of one call over [0, n), however
 * the walk is cut).  margin (n doubles, or NULL) receives the margins of the audited samples at their own indices.
 * Returns WG_ERR_BAD_ARG with nothing written for NULL audit, polys, t_start or t_end, NULL time, px or py with a sample to
 * audit, first_sample < 0, stride < 1, qcap < 1; and, with audit->status = WG_ERR_BAD_ARG and nothing else written, for a gait
 * the device calls refuse: n < 0, count < 0, first_sample > n, first_sample > 0 with audit->status != WG_OK.  count == 0 is not
 * a refusal: every sample is uncovered. */
int wg_zmp_audit(int first_sample, int n, const double *time, const double *px, const double *py, int stride, int count,
                 int qcap, const wg_zmp_polytope_t *polys, const double *t_start, const double *t_end, wg_zmp_audit_t *audit,
                 double *margin);
/* The same for B gaits on the device.  All pointers are DEVICE pointers; asynchronous on hip_stream.
 *   length     B      samples of each gait; nothing at or past length[b] is read or written
 *   time       lcap   ONE array shared by every gait, as for the foot-constraints calls
 *   px_tm, py_tm, pitch   sample k of gait b at [k * pitch + b]:  pitch = B reads zmp_x_tm / zmp_y_tm (wg_zmpdisc_*,
 *              wg_morisawa_*);  pitch = 2 B with py_tm = px_tm + B reads the preview's zmp2_tm [L][2][B];  pitch = 6 B with
 *              py_tm = px_tm + B reads the ground projection of com_tm
 *   queues, t_start, t_end [B][qcap], count B   what wg_foot_constraints_batch_dev / _append_dev / _fleet_dev wrote; only the
 *              first min(count[b], qcap) entries exist
 *   audit      B      the verdicts;  margin_tm  [lcap][B] or NULL: margin_tm[k * B + b] for k < length[b]
 * Per gait the bytes of wg_zmp_audit(0, length[b], ...).  A gait is refused -- audit[b].status = WG_ERR_BAD_ARG, nothing else
 * of it written, a neighbour never notices -- for length[b] < 0 (a gait a producer refused), length[b] > lcap, count[b] < 0.
 * Host-side errors (WG_ERR_BAD_ARG, nothing launched): a NULL input, B < 0, lcap < 1, qcap < 1, pitch < B;  B == 0 is WG_OK.
 * The time axis is split across blocks (chunks of wg_foot_constraints_chunk() samples); the per-chunk partial results live in
 * a buffer of the context between the two kernels and are folded in chunk order -- the first sample to attain the least margin
 * does not depend on the grid -- so launches of one context are ordered like the foot-constraints launches. */
int wg_zmp_audit_dev(int B, int lcap, const int *length, const double *time, const double *px_tm, const double *py_tm,
                     long long pitch, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end,
                     const int *count, wg_zmp_audit_t *audit, double *margin_tm, void *hip_stream);
/* The same on line, behind wg_foot_constraints_append_dev: audits the samples [done[b], length[b]), folds them into audit[b] and
 * margin_tm, and sets done[b] = length[b].  done[b] == 0 starts a gait's audit: audit[b] is ignored on input.
 * CONTRACT: after the call, audit[b] is byte for byte what wg_zmp_audit_dev writes for length[b] samples against the same queue.
 * This holds after every call, however the walk is cut (the least margin, the first sample and row to attain it and the counts
 * fold exactly), and on a queue still growing under wg_foot_constraints_append_dev: its provisional last t_end is
 * time[length[b] - 1], so every sample below length[b] has its final entry.
 *   length[b] == done[b]    the gait sits the call out: none of its bytes is touched.
 *   refused, with audit[b].status = WG_ERR_BAD_ARG, done[b] unchanged and nothing else written:  length[b] < 0 (a gait
 *       wg_zmpdisc_* refused);  length[b] > lcap;  count[b] < 0;  done[b] < 0;  done[b] > length[b];  done[b] < first_sample;
 *       done[b] > 0 with audit[b].status != WG_OK -- errors are sticky through the status.  A neighbour never notices.
 *   first_sample   a HOST-side lower bound on every done[b] (0 is always valid): the chunks of the time axis that lie wholly
 *       below it are not launched, so that a long walk does not pay a grid over its past.
 * Host-side errors as above, and NULL done or first_sample < 0.  Launches are ordered per context exactly like the batch
 * call's (the same buffer of the context). */
int wg_zmp_audit_append_dev(int B, int lcap, int first_sample, int *done, const int *length, const double *time,
                            const double *px_tm, const double *py_tm, long long pitch, int qcap,
                            const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count,
                            wg_zmp_audit_t *audit, double *margin_tm, void *hip_stream);

/* The queue walk of one tick, BuildConstraintMatrices (ZMPConstrainedQPFastFormulation.cpp:785-796, 822-835), for B gaits:
 * the first entry q with t_start[q] <= t0 <= t_end[q] is the start; for i = 0 .. N-1, q advances by one when
 * t0 + i T > t_end[q] (the reference's StartingTime + i*T); polys[b][i] is a copy of entry q.  N and T are the configured
 * Dimitrov model's (wg_dimitrov_configure).  Only the first min(count[b], qcap) entries of a queue exist.
 * The reference gives up when t0 lies in no interval or the walk passes the last entry (:800-804, :830-833); a fleet launch
 * cannot give up for one gait: such a gait gets its LAST polytope for the remaining instants (at rest on its final support,
 * the convention of wg_zmpdisc_batch_dev past a gait's length) and ran_out[b] = 1, otherwise 0; count[b] <= 0: zeroed
 * polytopes and ran_out[b] = 1.
 *   polys  [B][N], what wg_dimitrov_tick_batch_dev reads;  ran_out  B or NULL */
int wg_dimitrov_select_polys_dev(int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end,
                                 const int *count, double t0, wg_zmp_polytope_t *polys, int *ran_out, void *hip_stream);
/* n_ticks ticks of a fleet with nothing crossing the bus: for k = 0 .. n_ticks-1 { select at t; the launch of
 * wg_dimitrov_tick_batch_dev; t += T }, t starting at t0 and accumulated by repeated addition like the loop of
 * BuildZMPTrajectoryFromFootTrajectory (:1189-1192), all enqueued on hip_stream without a host synchronisation -- the bytes of
 * a host loop of wg_dimitrov_select_polys_dev + wg_dimitrov_tick_batch_dev, in every solver mode.  The B x N selected
 * polytopes live in a buffer of the context, sized on first use (growing never frees what a launch in flight may be reading,
 * as for wg_mpc_reserve); walks of one context on different streams are ordered like tick launches.
 *   outs     n_ticks x B, tick-major, or NULL;  ran_out  B: 1 once any tick of the gait ran out, or NULL.  ran_out is CLEARED
 *            by every walk call: a caller that walks in pieces (below) ORs it across its calls. */
int wg_dimitrov_walk_dev(int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end,
                         const int *count, double t0, int n_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs,
                         int *ran_out, int max_iter, void *hip_stream);
/* Continuing a walk (host arithmetic on the configured model's N and T; no launch).
 * wg_dimitrov_walk_time(t0, n_ticks) is the t at which tick n_ticks of a walk started at t0 selects: the walk's own repeated
 * addition of T, so the walks (t0, n1) and (wg_dimitrov_walk_time(t0, n1), n2) on the same states are the walk (t0, n1 + n2) bit
 * for bit (the product t0 + n T is another number).  NaN without a configured model.
 * wg_dimitrov_walk_safe_ticks(t0, t_have) is the largest n such that every tick k < n, at t = wg_dimitrov_walk_time(t0, k), has
 * t + (N - 1) T <= t_have -- the select kernel's own expression t0 + i * T at its last instant.  With t_have = time[length - 1]
 * of a gait that is still walking (the smallest over the fleet), such a tick selects from the provisional queue
 * wg_foot_constraints_append_dev has left what it will select from the final one: every entry but the last is final; the last
 * one's t_end is provisional, equals t_have and only grows; the tick's start test t_start <= t <= t_end and its N advance
 * tests t + i T > t_end compare against it only with instants <= t_have, which no later, larger t_end answers differently; and
 * a walk that never passes the last entry never sees the entries later calls add behind it.  A gait whose walk has ended
 * (wg_zmpdisc_end_dev, then one more wg_foot_constraints_append_dev) has a final queue and constrains nothing.  Negative code:
 * no configured model, or a t0 / t_have that is not finite. */
double wg_dimitrov_walk_time(double t0, int n_ticks);
int wg_dimitrov_walk_safe_ticks(double t0, double t_have);

/* The walk that follows each gait's own queue: a clock and a tick count per gait ------------------------------------------
 *
 * wg_dimitrov_follow_dev is wg_dimitrov_walk_dev with a range per gait, driven by the arrays the on-line calls leave on the
 * device: the host keeps no mirror of the gaits' sample counts, takes no minimum over them and reads nothing back, whatever
 * the gaits' step counts are and whenever each of them began, is fed or ends.  All pointers are DEVICE pointers.
 *   queues, t_start, t_end, count   [B][qcap] and B, as in wg_dimitrov_walk_dev (what wg_foot_constraints_append_dev grows)
 *   time     lcap             the array wg_foot_constraints_append_dev was given
 *   have     B                samples gait b's queue covers: that call's `done` array
 *   walk     B or NULL        the wg_zmpdisc state blobs: tell a gait whose walk has ended, and whose queue is therefore final
 *   flags    WG_DIMITROV_FOLLOW_ALL_FINAL: every queue is final (walk is not read)
 *   clock    B, in/out        the t at which the gait's next tick selects
 *   ticks    B, in/out        ticks the gait has behind it; 0 starts a walk from whatever states[b] holds
 *   outs     [tick_cap][B] or NULL, ABSOLUTE rows: tick k of gait b goes to outs[k * B + b]
 *   ran_out  B or NULL        ORed: set where a tick of the gait ran out, NEVER cleared by this call (clear it before the walk)
 * The call runs max_ticks rounds.  In each round, for every gait b, with N and T the configured Dimitrov model's:
 *   final(b) = flags & WG_DIMITROV_FOLLOW_ALL_FINAL, or walk != NULL && walk[b].ended && !walk[b].error &&
 *              walk[b].n_samples == have[b]          (ended, and the queue has consumed the end phase)
 *   go(b)    = ticks[b] < tick_cap && (final(b) || clock[b] + (N - 1) * T <= time[have[b] - 1])
 *              -- the select kernel's own expression t0 + i * T at i = N - 1, the one wg_dimitrov_walk_safe_ticks uses.
 * A gait that goes selects at t = clock[b] (the bytes wg_dimitrov_select_polys_dev gives for t0 = clock[b]), runs the tick of
 * wg_dimitrov_tick_batch_dev on states[b], writes its out struct to row ticks[b], then clock[b] += T and ticks[b] += 1: the
 * walk's repeated addition, clock[b] == wg_dimitrov_walk_time(clock0[b], ticks[b]) bit for bit.  Of a gait that does not go the
 * round touches no byte.
 *   sits the whole call out, nothing touched:  ticks[b] < 0 (errors are sticky through it), count[b] <= 0 (a gait
 *       wg_zmpdisc_* or the queue calls refused, or no queue yet), have[b] <= 0, or no round with go(b).
 *   refused (tested behind those three):  ticks[b] > tick_cap, have[b] > lcap, a clock[b] that is not finite:
 *       ticks[b] = WG_ERR_BAD_ARG and nothing else of the gait is written.  A neighbour never notices.
 * CONTRACT: after any sequence of follow calls interleaved with calls that grow `have`, and for any cut into max_ticks,
 * states[b], rows [0, ticks[b]) of outs and ran_out[b] (as an OR) are byte for byte what ONE wg_dimitrov_walk_dev(t0 = the gait's
 * initial clock, n_ticks = ticks[b]) over the gait's FINAL queue leaves for that gait; rows >= ticks[b] are untouched.
 * Why, per gait (the argument of wg_dimitrov_walk_safe_ticks with t_have = time[have[b] - 1] of this gait alone): every entry of
 * the gait's provisional queue but the last is final; the last one's t_end is provisional, equals time[have[b] - 1] and only grows;
 * a tick that goes compares it -- in the start test t_start <= t <= t_end and the N advance tests t + i T > t_end -- only with
 * instants <= time[have[b] - 1], which no later, larger t_end answers differently; and a walk that never passes the last entry
 * never sees the entries later calls add behind it.  A gait that is final has nothing provisional.  No gait's decision reads
 * anything of another gait.
 * Host-side errors (WG_ERR_BAD_ARG, nothing launched): no wg_dimitrov_configure; B < 0, qcap < 1, lcap < 1, tick_cap < 0,
 * max_ticks < 0; a NULL among queues, t_start, t_end, count, time, have, clock, ticks, states; unknown flag bits.  B == 0 or
 * max_ticks == 0 is WG_OK.  Asynchronous on hip_stream: 2 max_ticks launches, a round in which no gait goes included (the host
 * does not know).  The selected polytopes and one int per gait (the row its tick writes, or -1) live in the context's walk buffer:
 * follow calls and walks of one context are ordered like walks.  In the QL modes the longest-solve-first start order stays
 * scheduling only; a gait that sits a round out keeps its previous iteration count.
 * Added without a change of wg_abi_version(): detect by symbol. */
#define WG_DIMITROV_FOLLOW_ALL_FINAL 1
int wg_dimitrov_follow_dev(int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end,
                           const int *count, int lcap, const double *time, const int *have,
                           const wg_zmpdisc_state_t *walk, int flags, double *clock, int *ticks, int tick_cap, int max_ticks,
                           wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream);

/* Dimitrov-2008 fleets with a model per gait ------------------------------------------------------------------------------
 *
 * wg_dimitrov_configure gives a context one model.  A fleet whose gaits differ in CoM height or in the cost weights alpha,
 * beta -- robots of different size, a load sweep, a Monte-Carlo run over the weights -- carries its models as BLOCKS instead:
 * one opaque block of wg_dimitrov_constants_bytes() bytes (a multiple of 128) per model, the constants InitConstants leaves
 * behind (what wg_dimitrov_configure uploads) and zeros behind them, so that blocks compare as bytes.  The arithmetic is one
 * text (csrc/wg_dimitrov_math.hpp) compiled for the host and for the device: host blocks and device blocks are the same bytes.
 *
 * wg_dimitrov_constants(model, block): host arithmetic, no device call.  WG_ERR_BAD_ARG and an ALL-ZERO block for a model that
 *   does not exist: N outside 1 .. WG_PLDP_N, an unknown solver, T <= 0, a T, height, alpha or beta that is not finite, an LQ
 *   factor or an inverse of Pu that does not exist.  (T / Tctrl is not tested: Tctrl only spaces the samples of an out struct.)
 * wg_dimitrov_constants_unpack(block, ...): host arithmetic on a HOST copy of a block -- the arrays of
 *   wg_dimitrov_get_constants (iLQ, OptB, OptC, Pu, iPu, Px), of wg_dimitrov_get_qld_constants (Q, OptBq, OptCq, PuT) and
 *   iPuPx (2N x 6, PLDPSolver::PrecomputeiPuPx), at the sizes of the block's own N; model, if not NULL, gets N, solver, T,
 *   Tctrl and com_height (the weights are not kept: zeros).  Any pointer but block may be NULL.  WG_ERR_BAD_ARG for a failed
 *   (all-zero) block.
 * wg_dimitrov_constants_batch_dev(M, base, com_height, alpha, beta, blocks, status, hip_stream): M models on the device, one
 *   wavefront per model.
 *     base        read on the HOST: N, solver, T and Tctrl of every model, and the value of each per-model array that is NULL
 *     com_height, alpha, beta   DEVICE arrays of M doubles, or NULL
 *     blocks      M blocks, DEVICE;   status  M ints, DEVICE
 *   status[m] is WG_OK or WG_ERR_BAD_ARG, exactly what wg_dimitrov_constants returns for model m (a height or weight that is
 *   not finite included); a failed model gets an all-zero block, never a NaN, and no model touches a byte of another's.
 *   Asynchronous on hip_stream; keeps nothing in the context.  wg_dimitrov_constants_batch is the same call with HOST
 *   pointers, staged through the context's stream like the other host forms.
 *
 * The fleet descriptor: blocks points to M blocks and model_of to an int per gait, both on the DEVICE; the struct itself is read
 * on the host.  N, solver and T are fleet-wide (the select kernels and the kernel shapes are): a block made for another N is
 * refused like a failed one.
 *
 * wg_dimitrov_tick_fleet_dev / _walk_fleet_dev / _follow_fleet_dev are wg_dimitrov_tick_batch_dev / _walk_dev / _follow_dev
 * with the fleet after B: gait g runs with blocks[model_of[g]].  They read nothing of the context's configured Dimitrov model
 * (no wg_dimitrov_configure is needed) and use the context's walk buffers, launch ordering and longest-solve-first order
 * exactly as their twins do, through the same launcher.
 * CONTRACT: gait g of a fleet launch leaves, byte for byte, the state, outs rows, ran_out, clocks and tick counts that a context
 * configured with model model_of[g] leaves for it through the twin call.
 * A gait whose model_of[g] is outside [0, M), or whose block is a failed one, is refused: each of its ticks writes
 * ret = WG_PLDP_BAD_INPUT and n_iter = 0 into its out struct (if any) and nothing else -- no byte of its state changes, in a
 * walk or a follow call it sits every round's tick out (the follow select kernel, which knows no models, still counts the round
 * in clock[g] and ticks[g]), and no other gait notices.
 * Host-side refusals (WG_ERR_BAD_ARG before any device call): a NULL fleet, blocks, model_of or base; M < 1; B < 0; N outside
 * 1 .. WG_PLDP_N; an unknown solver; T <= 0; and whatever the twin call refuses.  B == 0 is WG_OK.
 * Added without a change of wg_abi_version(): detect by symbol. */
typedef struct wg_dimitrov_fleet {
  int N, solver, M, pad_;
  double T, Tctrl;
  const void *blocks;
  const int *model_of;
} wg_dimitrov_fleet_t;
size_t wg_dimitrov_constants_bytes(void);
int wg_dimitrov_constants(const wg_dimitrov_model_t *model, void *block);
int wg_dimitrov_constants_unpack(const void *block, wg_dimitrov_model_t *model, double *iLQ, double *OptB, double *OptC,
                                 double *Pu, double *iPu, double *Px, double *Q, double *OptBq, double *OptCq, double *PuT,
                                 double *iPuPx);
int wg_dimitrov_constants_batch_dev(int M, const wg_dimitrov_model_t *base, const double *com_height, const double *alpha,
                                    const double *beta, void *blocks, int *status, void *hip_stream);
int wg_dimitrov_constants_batch(int M, const wg_dimitrov_model_t *base, const double *com_height, const double *alpha,
                                const double *beta, void *blocks, int *status);
int wg_dimitrov_tick_fleet_dev(int B, const wg_dimitrov_fleet_t *fleet, const wg_zmp_polytope_t *polys,
                               wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter, void *hip_stream);
int wg_dimitrov_walk_fleet_dev(int B, const wg_dimitrov_fleet_t *fleet, int qcap, const wg_zmp_polytope_t *queues,
                               const double *t_start, const double *t_end, const int *count, double t0, int n_ticks,
                               wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter,
                               void *hip_stream);
int wg_dimitrov_follow_fleet_dev(int B, const wg_dimitrov_fleet_t *fleet, int qcap, const wg_zmp_polytope_t *queues,
                                 const double *t_start, const double *t_end, const int *count, int lcap, const double *time,
                                 const int *have, const wg_zmpdisc_state_t *walk, int flags, double *clock, int *ticks,
                                 int tick_cap, int max_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs,
                                 int *ran_out, int max_iter, void *hip_stream);

/* Herdt-2010 fleets with a model per gait ------------------------------------------------------------------------------------
 *
 * wg_mpc_configure gives a context one model.  A fleet whose gaits differ in their models -- robots of different size, a load
 * sweep over com_height_qp, a Monte-Carlo run over alpha / beta / gamma, sole sizes, margins, hip limits and step timing drawn
 * per gait -- carries them as BLOCKS instead: one opaque block of wg_mpc_block_bytes() bytes per model (76 032 bytes, a multiple
 * of 128, whatever N is: the tables are laid out for the largest horizon), holding the wg_model_t as given, the tick tables
 * wg_mpc_configure uploads behind it (S, U, Q_b, the packed factor R2 of blockdiag(Q_b, Q_b), its inverse Z2, the diagonal test,
 * the cross-block sign words) and zeros everywhere else, so that blocks compare as bytes.  The arithmetic is one text
 * (csrc/wg_tick_tables_math.hpp) compiled for the host and for the device: host blocks and device blocks are the same bytes.
 * When the constant block has no factor (blocks_ok == 0: the diagonal test or a pivot fails) R2, Z2 and the sign words are zero;
 * the tick then factors every QP itself, as it does for a configured model.
 *
 * wg_mpc_block(model, block): host arithmetic, no device call.  WG_ERR_BAD_ARG and an ALL-ZERO block for a model that is refused:
 *   whatever wg_mpc_configure refuses (N outside 2 .. 32, T / Tctrl != 20, more than four previewed steps); either
 *   WG_FLAG_GRAMIAN_MFMA_* flag (not available to fleets); a T, Tctrl, com_height_qp, alpha, beta, gamma or step_period that is not
 *   finite.  The compact view's WG_QL_SUMS / WG_QL_NORMS knobs are read from the environment at the call, as wg_mpc_configure does.
 * wg_mpc_block_unpack(block, ...): host arithmetic on a HOST copy of a block -- the model and the arrays at the block's own N
 *   (Sv, Sz: N x 3; Uv, Uz, Qb: N x N row-major; R2: 2N (2N + 1) / 2, packed by columns; Z2: 2N x 2N column-major).  Any pointer
 *   but block may be NULL.  WG_ERR_BAD_ARG for a refused (all-zero) block.
 * wg_mpc_blocks_batch_dev(M, models, blocks, status, hip_stream): M models (DEVICE array of wg_model_t) into M blocks (DEVICE),
 *   one wavefront per model; status[m] (DEVICE) is what wg_mpc_block returns for model m.  Every byte of block m is written once,
 *   by its own wavefront; a refused model gets an all-zero block, never a NaN.  Asynchronous on hip_stream; keeps nothing in the
 *   context.  wg_mpc_blocks_batch is the same call with HOST pointers, staged through the context's stream.
 *
 * The fleet descriptor is read on the host; blocks (M of them) and model_of (an int per gait) are DEVICE pointers.  `base`
 * decides the launch plan -- the problem view, the LDS and slot sizes, the column cap -- exactly as wg_mpc_configure(base) would;
 * it need not be one of the models.
 *
 * wg_mpc_tick_fleet_dev / wg_mpc_run_fleet_dev are wg_mpc_tick_batch_dev / wg_mpc_run_sched_dev with the fleet after B: gait g
 * runs with blocks[model_of[g]], its model fields and its tables.  They read nothing of the context's configured model (no
 * wg_mpc_configure is needed) and go through the same launcher as their twins: the context's slots, run buffer and launch
 * ordering, the longest-solve-first order, wg_mpc_reserve's sizing.  The run form always hands gaits over inside an XCD;
 * vref_sched == NULL is the unstaged run (wg_mpc_run_batch_dev).
 * CONTRACT: gait g of a fleet launch leaves, byte for byte, the state, outs rows, diag rows and hist row that a context
 * configured with model model_of[g] leaves for it through the twin call -- whichever view the fleet runs in.
 * One launch shape: a gait is accepted when model_of[g] is in [0, M), its block is a good one, its N, T and Tctrl equal base's
 * bit for bit, and its model is within the plan's step capacity: a compact plan (N == 16 and N T <= 2 step_period + 1e-12 for
 * base) holds two previewed steps and accepts only models for which the same inequality holds; every other plan is sized for
 * four and accepts all.  Any other gait is REFUSED: each of its ticks writes ifail = WG_IFAIL_NO_MODEL and five zeros into its
 * six diagnostic ints (its diag row, and its out struct if there is one), 0 into the iteration count that orders the next
 * launch, and nothing else -- no byte of its state changes (no clock advance, no staged reference), in a run launch it sits every
 * tick out, and no other gait notices.
 * Host-side refusals (WG_ERR_BAD_ARG before any device call): a NULL fleet, blocks or model_of; M < 1; B < 0; a base that
 * wg_mpc_block would refuse; whatever the twin refuses.  B == 0 is WG_OK.
 * Added without a change of wg_abi_version(): detect by symbol. */
#define WG_IFAIL_NO_MODEL (-1)       /* QL's own codes are >= 0 */
typedef struct wg_mpc_fleet {
  wg_model_t base;
  int M, pad_;
  const void *blocks;
  const int *model_of;
} wg_mpc_fleet_t;
size_t wg_mpc_block_bytes(void);
int wg_mpc_block(const wg_model_t *model, void *block);
int wg_mpc_block_unpack(const void *block, wg_model_t *model, double *Sv, double *Sz, double *Uv, double *Uz, double *Qb,
                        double *R2, double *Z2, double *diag_b, int *blocks_ok);
int wg_mpc_blocks_batch_dev(int M, const wg_model_t *models, void *blocks, int *status, void *hip_stream);
int wg_mpc_blocks_batch(int M, const wg_model_t *models, void *blocks, int *status);
int wg_mpc_tick_fleet_dev(int B, const wg_mpc_fleet_t *fleet, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag,
                          int advance_calls, int *hist, int hist_cap, int *hist_len, void *hip_stream);
int wg_mpc_run_fleet_dev(int B, const wg_mpc_fleet_t *fleet, wg_gait_state_t *states, int n_ticks, int advance_calls,
                         const double *vref_sched, int period, wg_tick_out_t *outs, int *diag, void *hip_stream);

/* Invariant Hessian block on the matrix cores, batched over models -----------------------------------------------------
 *
 * wg_gramian_batch computes, for B models that differ in QP sampling period T[b] and CoM height h[b],
 *     Q_b = beta I + alpha Uv'Uv + gamma Uz'Uz      (N x N, row-major, one block after the other)
 * i.e. GeneratorVelRef::build_invariant_part (src/ZMPRefTrajectoryGeneration/generator-vel-ref.cpp:587-614) on the maps
 * of RigidBodySystem::compute_dyn_cjerk (src/PreviewControl/rigid-body-system.cpp:377-452) -- the one GEMM-shaped step
 * of the path.  One wavefront per model; Uv and Uz are generated in registers from (T, h) and multiplied with
 * v_mfma_f64_16x16x4_f64 (WG_GRAMIAN_F64) or v_mfma_f32_16x16x4_f32 (WG_GRAMIAN_F32, operands rounded to float,
 * result widened).  The matrix cores fuse and reorder the sums: results match the host loop of wg_mpc_configure (which
 * keeps the reference's order, because the tick is bit-exact) to rounding only -- 1e-14 / 1e-6 relative. */
#define WG_GRAMIAN_F64 0
#define WG_GRAMIAN_F32 1
int wg_gramian_batch(int B, int N, const double *T, const double *h, double alpha, double beta, double gamma, int precision,
                     double *Qb);
int wg_gramian_batch_dev(int B, int N, const double *T, const double *h, double alpha, double beta, double gamma,
                         int precision, double *Qb, void *hip_stream);

/* Morisawa-2007 analytic walks: CoM, ZMP and feet of a step sequence in closed form, batched over gaits -----------------------
 *
 * What the reference computes after ":SetAlgoForZmpTrajectory Morisawa" for a ":stepseq" (no on-line change):
 *     AnalyticalMorisawaCompact::GetZMPDiscretization      src/ZMPRefTrajectoryGeneration/AnalyticalMorisawaCompact.cpp:514-579
 *       = BuildAndSolveCOMZMPForASetOfSteps (:360-512, IgnoreFirstRelativeFoot = true, DoNotPrepareLastFoot = false) with
 *         InitializeBasicVariables (:170-224), BuildingTheZMatrix / ComputeZ1 / ComputeZj / ComputeZm (:944-1164), ComputeW
 *         (:831-942), TransfertTheCoefficientsToTrajectories (:1166-1233), then FillQueues (:2230-2290; OnLine's analytic branch
 *         :648-723 evaluates the same),
 *     AnalyticalZMPCOGTrajectory::ComputeCOM / ComputeCOMSpeed / ComputeZMP by interval, GetIntervalIndexFromTime,
 *       TransfertOneIntervalCoefficientsFromCOGTrajectoryToZMPOne, Building3rdOrderPolynomial
 *                                                          src/Mathematics/AnalyticalZMPCOGTrajectory.cpp:175-196, 276-282,
 *                                                          472-507, 386-410, 425-456
 *     LeftAndRightFootTrajectoryGenerationMultiple::InitializeFromRelativeSteps (Continuity = false), SetAnInterval
 *                                                          src/FootTrajectoryGeneration/LeftAndRightFootTrajectoryGenerationMultiple.cpp:168-572, 107-166
 *     FootTrajectoryGenerationMultiple::Compute(t, FAP, index), FootTrajectoryGenerationStandard::
 *       SetParametersWithInitPosInitSpeed / ComputeAll     FootTrajectoryGenerationMultiple.cpp:128-135,
 *                                                          FootTrajectoryGenerationStandard.cpp:188-227, 307-333
 *     Polynome4::SetParametersWithInitPosInitSpeed, Polynome5::SetParameters(FT, FP, p0, v0, 0),
 *       Polynome3::SetParametersWithInitPosInitSpeed       src/Mathematics/PolynomeFoot.cpp:122-146, 226-240, 59-79
 * The walk of S steps has 2 S + 1 intervals (3 t_single, then t_double and t_single in turn, 3 t_single) and one linear system
 * Z y = w of n = 4 S + 8 unknowns per gait; x and y are two right-hand sides of one Z.  The reference hands it to LAPACK
 * (dgetrf_ / dgesvx_, :263-357); here it is a partially pivoted LU without refinement, so parity is by tolerance.  Not here: the
 * on-line window (InitOnLine, OnLineAddFoot, ChangeFootLandingPosition, TimeChange), the preview-control filter, ChangeOnLineStep,
 * a CoM height per interval.
 *
 * Two steps: wg_morisawa_solve* turns each gait's steps into a TRAJECTORY BLOCK of wg_morisawa_block_bytes(smax) bytes (counts,
 * interval times and omega_j, per interval the ZMP and CoG polynomials of x and y and the weights V, W, both feet's polynomials,
 * the ZMP profile, the absolute support feet, w and y, Z's LU factor and pivots -- a new right-hand side can be solved from the
 * block, and wg_morisawa_resolve* below does -- zeros elsewhere: blocks compare as bytes); wg_morisawa_sample* evaluates blocks on one clock.
 *   steps      B x smax   gait b uses the first n_steps[b]; 2 <= n_steps[b] <= smax <= WG_MORISAWA_MAX_STEPS.  sx, sy, theta
 *                         (degrees) are read; the times are the model's
 *   init_feet  B x 6      left x, y, theta, right x, y, theta at the start (z, omega, omega2 and every speed 0)
 *   com0       B x 3      start CoM x, y and height (lStartingCOMState; the height is every interval's CoMZ, ZMPZ is 0)
 *   blocks     B blocks;  status B: WG_OK or WG_MORISAWA_BAD_INPUT (n_steps out of range; a time or the height not finite or not
 *                         positive; another input not finite; an omega_j dT_j > WG_MORISAWA_WALK_ARG_MAX -- a bound of
 *                         accuracy: V cosh + W sinh cancels by e^(omega dT), so the method in float64, the reference's
 *                         arithmetic included, loses those digits; up to the bound 16 times the float64 restatement's
 *                         distance from the 50-digit one stays below 1e-8 m for gaits in the suite's ranges, measured by
 *                         tools/measure_morisawa_admission.py and filed as profiles/morisawa_admission.txt; a formulation that
 *                         stays accurate beyond it is later work.  cosh / sinh themselves are made for [0, 40]),
 *                         WG_MORISAWA_SINGULAR (a zero or non-finite pivot).  A refused gait's block is left untouched.
 * Sample k is at trajectory time t_start + k additions of T (the control loop's clock, PatternGeneratorInterfacePrivate.cpp:1256;
 * the reference's queue starts at 2 t_single); a gait has the samples with t <= the sum of its interval times (FillQueues' loop).
 * Outputs are time-major in the layouts of wg_zmpdisc_full_batch_dev: zmp_x_tm, zmp_y_tm [lcap][B]; com_tm [lcap][4][B] (x, dx,
 * y, dy); left_tm, right_tm [lcap][6][B] (x, y, z, theta, omega, omega2); left_type_tm, right_type_tm [lcap][B] (the interval's
 * nature, SetNatureInterval); any of them NULL.  Samples past a gait's length repeat its last one.  length[b] (may be NULL):
 * the count, or status[b] < 0 handed on (status may be NULL: every block is taken as solved), WG_MORISAWA_BAD_INPUT for a block
 * that is not one of this smax, WG_MORISAWA_CAPACITY for more samples than lcap; such a gait's outputs are left untouched.
 * Host-side errors (WG_ERR_BAD_ARG, nothing launched): NULL inputs, B < 0, smax outside [2, WG_MORISAWA_MAX_STEPS], lcap < 1,
 * T or t_start not finite, T <= 0, t_start < 0.  B == 0 is WG_OK.
 * wg_morisawa_solve, _solve_fleet, _sample, _length, _system are host arithmetic without a device call -- the kernels' bytes.
 * The _dev calls take DEVICE pointers and are asynchronous on hip_stream; wg_morisawa_walk_dev is solve and sample on that
 * stream without a synchronisation between them (T = model->T).  The _fleet forms take B models, gait b its own (host array for
 * wg_morisawa_solve_fleet, DEVICE array for the _dev forms): gait b's bytes are those of the one-model call handed model b. */
#define WG_MORISAWA_MAX_STEPS 14     /* n = 4 S + 8 = 64: one row of Z per lane */
#define WG_MORISAWA_WALK_ARG_MAX 13.5 /* the largest admitted omega_j dT_j: X* of profiles/morisawa_admission.txt */
#define WG_MORISAWA_BAD_INPUT (-1)
#define WG_MORISAWA_CAPACITY (-2)
#define WG_MORISAWA_SINGULAR (-3)
typedef struct wg_morisawa_model {
  double T;                           /* m_SamplingPeriod  0.005 */
  double t_single, t_double;          /* m_Tsingle, m_Tdble  0.78, 0.02 (CommonTools.cpp:57-67 of the reference's tests) */
  double step_height;                 /* m_StepHeight  0.07 */
  double omega;                       /* m_Omega, degrees  0 */
} wg_morisawa_model_t;
/* a block, read on the host: pointers into it */
typedef struct wg_morisawa_view {
  int n_steps, n_int, n, smax;        /* S, 2 S + 1, 4 S + 8, the smax the block was made for */
  double com_height, t_total;         /* CoMZ; the sum of the interval times */
  const double *dT, *omega, *tref;    /* [n_int] m_DeltaTj, m_Omegaj, m_RefTime */
  const double *zmp_x, *cog_x, *zmp_y, *cog_y;   /* [n_int][5] coefficients 0 .. 4 (interior intervals are cubics) */
  const double *Vx, *Wx, *Vy, *Wy;    /* [n_int] */
  const double *left, *right;         /* [n_int][6][6]: axis x y z theta omega omega2, coefficients 0 .. 5 */
  const int *left_type, *right_type;  /* [n_int] m_NatureOfIntervals */
  const double *profile_x, *profile_y;/* [n_int] ZMPProfil */
  const double *support;              /* [n_steps][3] m_AbsoluteSupportFootPositions x, y, theta (degrees) */
  const double *wx, *wy, *yx, *yy;    /* [n] */
  const int *piv;                     /* [n] row k was swapped with row piv[k] >= k (LAPACK's ipiv, 0-based) */
  const double *lu;                   /* P Z = L U, unit L below the diagonal; rows lu_pitch apart */
  int lu_pitch, pad_;                 /* a long block (wg_morisawa_long_block_unpack): lu_pitch = 16 and lu is the ROW BAND, entry
                                         (i, c) at lu[16 i + c - i + 5] for i - 5 <= c <= i + 9, with dgbtf2's multipliers: not
                                         swapped by later steps.  piv reads the same.  See wg_morisawa_long_* below */
} wg_morisawa_view_t;
#define WG_MORISAWA_MODEL_BYTES 40
#define WG_MORISAWA_VIEW_BYTES 232
#ifdef __cplusplus
static_assert(sizeof(wg_morisawa_model_t) == WG_MORISAWA_MODEL_BYTES, "wg_morisawa_model_t is part of the ABI");
static_assert(sizeof(wg_morisawa_view_t) == WG_MORISAWA_VIEW_BYTES, "wg_morisawa_view_t is part of the ABI");
#else
_Static_assert(sizeof(wg_morisawa_model_t) == WG_MORISAWA_MODEL_BYTES, "wg_morisawa_model_t is part of the ABI");
_Static_assert(sizeof(wg_morisawa_view_t) == WG_MORISAWA_VIEW_BYTES, "wg_morisawa_view_t is part of the ABI");
#endif
void wg_morisawa_defaults(wg_morisawa_model_t *model);
size_t wg_morisawa_block_bytes(int smax);                 /* a multiple of 128; 0 for an smax out of range */
int wg_morisawa_block_unpack(const void *block, int smax, wg_morisawa_view_t *view);
/* samples of a walk of n_steps steps from t_start, by the additions the sampler makes, or a negative code */
int wg_morisawa_length(const wg_morisawa_model_t *model, int n_steps, double t_start);
/* the library's cosh and sinh of x in [0, 40] (IEEE + - * / only, the same bits on host and device) */
int wg_morisawa_coshsinh(double x, double *cosh_x, double *sinh_x);
/* Z (n x n, rows n apart) and w of x and y before the elimination, one gait; returns n or a negative code */
int wg_morisawa_system(const wg_morisawa_model_t *model, int n_steps, const wg_rel_step_t *steps, const double *init_feet,
                       const double *com0, double *Z, double *wx, double *wy);
int wg_morisawa_solve(const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                      const double *init_feet, const double *com0, void *blocks, int *status);
int wg_morisawa_solve_fleet(const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                            const double *init_feet, const double *com0, void *blocks, int *status);
int wg_morisawa_sample(int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap,
                       double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm,
                       int *right_type_tm, int *length);
int wg_morisawa_solve_dev(const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                          const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream);
int wg_morisawa_solve_fleet_dev(const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps,
                                const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status,
                                void *hip_stream);
int wg_morisawa_sample_dev(int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap,
                           double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm,
                           double *right_tm, int *right_type_tm, int *length, void *hip_stream);
int wg_morisawa_walk_dev(const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                         const double *init_feet, const double *com0, void *blocks, int *status, double t_start, int lcap,
                         double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm,
                         double *right_tm, int *right_type_tm, int *length, void *hip_stream);
int wg_morisawa_walk_fleet_dev(const wg_morisawa_model_t *models, double T, int B, int smax, const wg_rel_step_t *steps,
                               const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status,
                               double t_start, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm,
                               int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream);

/* Morisawa walks of up to WG_MORISAWA_LONG_MAX_STEPS steps: a second family next to the first, wg_morisawa_long_* ---------------
 *
 * The same walk, the same arguments, statuses, refusals and outputs as the calls above with `_long` in the name; what differs is
 * how Z y = w is solved and what a block holds behind the pivots.  Z's non-zeros lie within 5 below and 4 above the diagonal
 * whatever S is, so the long family eliminates inside the band: the pivot of column k is looked for in rows k .. k + 5, a row
 * update covers columns k + 1 .. k + 9.  It takes the pivots of the dense elimination and gives the same values (products with
 * structural zeros are all it leaves out; a zero may differ in sign), so for smax <= WG_MORISAWA_MAX_STEPS the two families agree
 * by value in every sample.  A long block is wg_morisawa_long_block_bytes(smax) bytes: the short block's sections in the short
 * block's order up to the pivots, then the factor in ROW-BAND form, n rows 16 doubles apart: row i holds columns i - 5 .. i + 9
 * in its words 0 .. 14 (column c at word c - i + 5; what falls outside the matrix and word 15 are zero).  wg_morisawa_long_block_
 * unpack fills the same wg_morisawa_view_t with lu at the band and lu_pitch = 16.  The convention is LAPACK's dgbtf2: step k swaps
 * rows k and piv[k] over columns k .. k + 9 only, so the multipliers of column k (rows k + 1 .. k + 5, words left of the diagonal)
 * stay at the positions where they were made and are NOT swapped by later steps.  A new right-hand side b is solved as dgbtrs
 * does: for k = 0 .. n - 2 swap b[k] and b[piv[k]], then b[i] -= lu(i, k) b[k] for i = k + 1 .. min(n - 1, k + 5); then, for c from
 * n - 1 down, b[c] /= lu(c, c) and b[i] -= lu(i, c) b[c] for i = max(0, c - 9) .. c - 1.  The int at byte 32 of a long block (the
 * header's first word behind the two doubles, zero in a short block) is 1; wg_morisawa_long_sample* refuse a block without it
 * (WG_MORISAWA_BAD_INPUT), and a short block or one of another smax with it.  wg_morisawa_long_system writes Z before the
 * elimination in that row-band form, n x 16.  Blocks of the two families are not interchangeable. */
#define WG_MORISAWA_LONG_MAX_STEPS 64   /* n = 4 S + 8 = 264 */
size_t wg_morisawa_long_block_bytes(int smax);            /* a multiple of 128; 0 for an smax outside [2, 64] */
int wg_morisawa_long_block_unpack(const void *block, int smax, wg_morisawa_view_t *view);
int wg_morisawa_long_length(const wg_morisawa_model_t *model, int n_steps, double t_start);
int wg_morisawa_long_system(const wg_morisawa_model_t *model, int n_steps, const wg_rel_step_t *steps, const double *init_feet,
                            const double *com0, double *Zband, double *wx, double *wy);
int wg_morisawa_long_solve(const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                           const double *init_feet, const double *com0, void *blocks, int *status);
int wg_morisawa_long_solve_fleet(const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps,
                                 const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status);
int wg_morisawa_long_sample(int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap,
                            double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm,
                            double *right_tm, int *right_type_tm, int *length);
int wg_morisawa_long_solve_dev(const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                               const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream);
int wg_morisawa_long_solve_fleet_dev(const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps,
                                     const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status,
                                     void *hip_stream);
int wg_morisawa_long_sample_dev(int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap,
                                double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm,
                                double *right_tm, int *right_type_tm, int *length, void *hip_stream);
int wg_morisawa_long_walk_dev(const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                              const double *init_feet, const double *com0, void *blocks, int *status, double t_start, int lcap,
                              double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm,
                              double *right_tm, int *right_type_tm, int *length, void *hip_stream);
int wg_morisawa_long_walk_fleet_dev(const wg_morisawa_model_t *models, double T, int B, int smax, const wg_rel_step_t *steps,
                                    const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status,
                                    double t_start, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm,
                                    int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream);

/* Morisawa walks re-planned from a block's kept factor: wg_morisawa_resolve*, wg_morisawa_long_resolve* -------------------------
 *
 * Z depends on the interval times, the CoM height and the step count and on nothing else, so a solved block -- a FACTOR BLOCK --
 * serves every other plan on its timing, as the reference's kept dgetrf_ result does until ResetTheResolutionOfThePolynomial
 * (AnalyticalMorisawaCompact.cpp:263-357).  Given factor blocks and, per gait, a plan -- steps, initial feet, start CoM x and y --
 * these calls write the block that wg_morisawa_solve* (wg_morisawa_long_solve*) would write for that plan with the model, CoM
 * height and step count the gait's factor block was made with: every byte of it, the copies of dT, omega, tref, pivots and factor
 * included, so blocks still compare as bytes and wg_morisawa[_long]_sample* read them unchanged.  Z is not built and no pivot is
 * searched; both right-hand sides go through the stored factor, each entry meeting the products and differences of the full
 * solve in the full solve's order.  The whole walk is planned from t = 0; nothing here changes a walk under way.
 *   factors    n_factors blocks of this family and this smax (wg_morisawa[_long]_block_bytes(smax) apart)
 *   factor_of  B ints: the factor block of gait b; NULL: every gait uses block 0
 *   steps      B x smax   gait b uses as many as its factor block has steps: there is no n_steps
 *   init_feet, com0, blocks, status   as for wg_morisawa_solve; com0[b][2] must be the factor block's height
 * A gait is refused by itself, status WG_MORISAWA_BAD_INPUT and its block left untouched, when factor_of[b] is outside
 * [0, n_factors); when its factor block is not a solved block of this family and smax (a short block handed to the long call and
 * a long block handed to the short call among them, and a block whose pivots do not lie among their columns' rows); when the model's times do not give the block's interval times bit for bit;
 * when com0[b][2] is not the block's CoM height bit for bit; when an input is not finite, as wg_morisawa_solve tests it.
 * WG_MORISAWA_SINGULAR does not arise.  Host-side errors (WG_ERR_BAD_ARG, nothing launched): NULL inputs, B < 0, n_factors < 1,
 * smax outside the family's range.  B == 0 is WG_OK.
 * `blocks` must not overlap `factors`: a factor block is read while blocks are written; this is not checked.  Whether a factor
 * block is the one the caller means is the caller's business: a stale block that is still a valid block of these times and this
 * height gives the bytes of a solve with its header, which is what these calls promise.
 * wg_morisawa_resolve, _resolve_fleet and their long forms are host arithmetic without a device call; the _dev forms take DEVICE
 * pointers (the one-model forms the model on the host, by value into the launch, as wg_morisawa_solve_dev) and are asynchronous on
 * hip_stream: factor blocks made by wg_morisawa[_long]_solve_dev earlier on that stream need no synchronisation, and
 * wg_morisawa[_long]_sample_dev behind the call on that stream samples the new walks.
 * Added without a change of wg_abi_version(): detect by symbol. */
int wg_morisawa_resolve(const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors, const int *factor_of,
                        const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status);
int wg_morisawa_resolve_fleet(const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors,
                              const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                              void *blocks, int *status);
int wg_morisawa_resolve_dev(const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors,
                            const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                            void *blocks, int *status, void *hip_stream);
int wg_morisawa_resolve_fleet_dev(const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors,
                                  const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                                  void *blocks, int *status, void *hip_stream);
int wg_morisawa_long_resolve(const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors,
                             const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                             void *blocks, int *status);
int wg_morisawa_long_resolve_fleet(const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors,
                                   const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                                   void *blocks, int *status);
int wg_morisawa_long_resolve_dev(const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors,
                                 const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                                 void *blocks, int *status, void *hip_stream);
int wg_morisawa_long_resolve_fleet_dev(const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors,
                                       const int *factor_of, const wg_rel_step_t *steps, const double *init_feet,
                                       const double *com0, void *blocks, int *status, void *hip_stream);

/* The context forms of the entry points above (same arguments after the context, same semantics) ----------------------------
 *
 * Written out: those whose default-context form is more than a forward (a query that must not create the default context, or a
 * fleet call that refuses its arguments before the default context, and with it the device, is looked for). */
long long wg_overlap_serialised_ctx(wg_ctx_t *ctx);
size_t wg_mpc_tick_lds_bytes_ctx(wg_ctx_t *ctx);
int wg_preview_window_ctx(wg_ctx_t *ctx);
int wg_riccati_gains_batch_dev_ctx(wg_ctx_t *ctx, int B, double T, const double *zc, double Q, double R, int Nl, int mode,
                                   double *K_tm, double *F_tm, int *status, void *hip_stream);
int wg_riccati_gains_batch_ctx(wg_ctx_t *ctx, int B, double T, const double *zc, double Q, double R, int Nl, int mode,
                               double *K, double *F, int *status);
int wg_preview_run_fleet_dev_ctx(wg_ctx_t *ctx, int B, int L, const wg_preview_fleet_t *fleet, const double *zmp_x_tm,
                                 const double *zmp_y_tm, double *state, double *com_tm, double *zmp2_tm, int simulation,
                                 void *hip_stream);
int wg_preview_follow_fleet_dev_ctx(wg_ctx_t *ctx, int B, int lcap, const int *length, int *done,
                                    const wg_preview_fleet_t *fleet, const double *zmp_x_tm, const double *zmp_y_tm,
                                    double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream);
int wg_dimitrov_constants_batch_dev_ctx(wg_ctx_t *ctx, int M, const wg_dimitrov_model_t *base, const double *com_height,
                                        const double *alpha, const double *beta, void *blocks, int *status, void *hip_stream);
int wg_dimitrov_constants_batch_ctx(wg_ctx_t *ctx, int M, const wg_dimitrov_model_t *base, const double *com_height,
                                    const double *alpha, const double *beta, void *blocks, int *status);
int wg_dimitrov_tick_fleet_dev_ctx(wg_ctx_t *ctx, int B, const wg_dimitrov_fleet_t *fleet, const wg_zmp_polytope_t *polys,
                                   wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter, void *hip_stream);
int wg_dimitrov_walk_fleet_dev_ctx(wg_ctx_t *ctx, int B, const wg_dimitrov_fleet_t *fleet, int qcap,
                                   const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end,
                                   const int *count, double t0, int n_ticks, wg_dimitrov_state_t *states,
                                   wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream);
int wg_dimitrov_follow_fleet_dev_ctx(wg_ctx_t *ctx, int B, const wg_dimitrov_fleet_t *fleet, int qcap,
                                     const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end,
                                     const int *count, int lcap, const double *time, const int *have,
                                     const wg_zmpdisc_state_t *walk, int flags, double *clock, int *ticks, int tick_cap,
                                     int max_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out,
                                     int max_iter, void *hip_stream);
/* Every other one, one entry X(ret, name, (params), (args)) each: this header makes the prototype `ret name_ctx(wg_ctx_t *ctx, params);`
 * of it, the library the forwarder `ret name(params) { return name_ctx(<the default context>, args); }` (wrong params: no build). */
#define WG_CTX_FORWARDED(X) \
  X(int, wg_qp_solve_batch_dev, (int B, int nmax, int mmax, const int *n, const int *m, const int *me, const double *C, const double *d, const double *A, \
    const double *b, const double *xl, const double *xu, double eps, double *x, double *u, int *ifail, int *n_iter, int *iact, int *nact, int *hist, \
    int hist_cap, int *hist_len, void *hip_stream), (B, nmax, mmax, n, m, me, C, d, A, b, xl, xu, eps, x, u, ifail, n_iter, iact, nact, hist, hist_cap, \
    hist_len, hip_stream)) \
  X(int, wg_qp_solve_batch, (int B, int nmax, int mmax, const int *n, const int *m, const int *me, const double *C, const double *d, const double *A, \
    const double *b, const double *xl, const double *xu, double eps, double *x, double *u, int *ifail, int *n_iter, int *iact, int *nact, int *hist, \
    int hist_cap, int *hist_len), (B, nmax, mmax, n, m, me, C, d, A, b, xl, xu, eps, x, u, ifail, n_iter, iact, nact, hist, hist_cap, hist_len)) \
  X(int, wg_set_overlap_strict, (int on), (on)) \
  X(int, wg_mpc_configure, (const wg_model_t *model), (model)) \
  X(int, wg_mpc_reserve, (int max_gaits), (max_gaits)) \
  X(int, wg_mpc_tick_batch_dev, (int B, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls, int *hist, int hist_cap, int *hist_len, \
    void *hip_stream), (B, states, outs, diag, advance_calls, hist, hist_cap, hist_len, hip_stream)) \
  X(int, wg_mpc_run_batch_dev, (int B, wg_gait_state_t *states, int n_ticks, int advance_calls, wg_tick_out_t *outs, int *diag, void *hip_stream), (B, \
    states, n_ticks, advance_calls, outs, diag, hip_stream)) \
  X(int, wg_mpc_run_sched_dev, (int B, wg_gait_state_t *states, int n_ticks, int advance_calls, const double *vref_sched, int period, wg_tick_out_t *outs, \
    int *diag, void *hip_stream), (B, states, n_ticks, advance_calls, vref_sched, period, outs, diag, hip_stream)) \
  X(int, wg_mpc_tick_batch, (int B, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls, int *hist, int hist_cap, int *hist_len), (B, \
    states, outs, diag, advance_calls, hist, hist_cap, hist_len)) \
  X(int, wg_mpc_set_velref_dev, (int B, wg_gait_state_t *states, const double *vref, void *hip_stream), (B, states, vref, hip_stream)) \
  X(int, wg_mpc_tick_pinned, (wg_gait_state_t *state, wg_tick_out_t *out, int *diag, int advance_calls), (state, out, diag, advance_calls)) \
  X(int, wg_mpc_assemble_batch, (int B, const wg_gait_state_t *states, int advance_calls, int nmax, int mmax, double *C, double *d, double *A, double *b, \
    double *xl, double *xu, int *n, int *m), (B, states, advance_calls, nmax, mmax, C, d, A, b, xl, xu, n, m)) \
  X(int, wg_mpc_assemble_batch_dev, (int B, const wg_gait_state_t *states, int advance_calls, int nmax, int mmax, double *C, double *d, double *A, double *b, \
    double *xl, double *xu, int *n, int *m, void *hip_stream), (B, states, advance_calls, nmax, mmax, C, d, A, b, xl, xu, n, m, hip_stream)) \
  X(int, wg_pldp_configure, (int N, const double *iPu, const double *Px, const double *Pu), (N, iPu, Px, Pu)) \
  X(int, wg_pldp_solve_batch_dev, (int B, int mcap, const int *m, const double *D, const double *A, const double *b, const double *zmpref, \
    const double *xkyk, const int *similar, const int *n_removed, const int *starting, int max_iter, wg_pldp_state_t *states, double *X, int *ret, \
    int *n_iter, int *active, int *n_active, void *hip_stream), (B, mcap, m, D, A, b, zmpref, xkyk, similar, n_removed, starting, max_iter, states, X, ret, \
    n_iter, active, n_active, hip_stream)) \
  X(int, wg_pldp_solve_batch, (int B, int mcap, const int *m, const double *D, const double *A, const double *b, const double *zmpref, const double *xkyk, \
    const int *similar, const int *n_removed, const int *starting, int max_iter, wg_pldp_state_t *states, double *X, int *ret, int *n_iter, int *active, \
    int *n_active), (B, mcap, m, D, A, b, zmpref, xkyk, similar, n_removed, starting, max_iter, states, X, ret, n_iter, active, n_active)) \
  X(int, wg_dimitrov_configure, (const wg_dimitrov_model_t *model), (model)) \
  X(int, wg_dimitrov_get_constants, (double *iLQ, double *OptB, double *OptC, double *Pu, double *iPu, double *Px), (iLQ, OptB, OptC, Pu, iPu, Px)) \
  X(int, wg_dimitrov_get_qld_constants, (double *Q, double *OptB, double *OptC, double *PuT), (Q, OptB, OptC, PuT)) \
  X(int, wg_dimitrov_tick_batch_dev, (int B, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter, \
    void *hip_stream), (B, polys, states, outs, max_iter, hip_stream)) \
  X(int, wg_dimitrov_tick_batch, (int B, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter), (B, polys, \
    states, outs, max_iter)) \
  X(int, wg_foot_constraints_batch_dev, (int B, int lcap, const int *length, const double *time, const double *left_tm, const int *left_type_tm, \
    const double *right_tm, double sole_w, double sole_h, double constraint_x, double constraint_y, int qcap, wg_zmp_polytope_t *queues, double *t_start, \
    double *t_end, int *count, void *hip_stream), (B, lcap, length, time, left_tm, left_type_tm, right_tm, sole_w, sole_h, constraint_x, constraint_y, qcap, \
    queues, t_start, t_end, count, hip_stream)) \
  X(int, wg_foot_constraints_append_dev, (int B, int lcap, int first_sample, int *done, const int *length, const double *time, const double *left_tm, \
    const int *left_type_tm, const double *right_tm, double sole_w, double sole_h, double constraint_x, double constraint_y, int qcap, \
    wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream), (B, lcap, first_sample, done, length, time, left_tm, \
    left_type_tm, right_tm, sole_w, sole_h, constraint_x, constraint_y, qcap, queues, t_start, t_end, count, hip_stream)) \
  X(double, wg_dimitrov_walk_time, (double t0, int n_ticks), (t0, n_ticks)) \
  X(int, wg_dimitrov_walk_safe_ticks, (double t0, double t_have), (t0, t_have)) \
  X(int, wg_dimitrov_select_polys_dev, (int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, \
    double t0, wg_zmp_polytope_t *polys, int *ran_out, void *hip_stream), (B, qcap, queues, t_start, t_end, count, t0, polys, ran_out, hip_stream)) \
  X(int, wg_dimitrov_walk_dev, (int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, double t0, \
    int n_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream), (B, qcap, queues, t_start, t_end, \
    count, t0, n_ticks, states, outs, ran_out, max_iter, hip_stream)) \
  X(int, wg_dimitrov_follow_dev, (int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, int lcap, \
    const double *time, const int *have, const wg_zmpdisc_state_t *walk, int flags, double *clock, int *ticks, int tick_cap, int max_ticks, \
    wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream), (B, qcap, queues, t_start, t_end, count, lcap, time, \
    have, walk, flags, clock, ticks, tick_cap, max_ticks, states, outs, ran_out, max_iter, hip_stream)) \
  X(int, wg_preview_configure, (const wg_preview_gains_t *gains, const double *F), (gains, F)) \
  X(int, wg_preview_run_batch_dev, (int B, int L, const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm, double *zmp2_tm, \
    int simulation, void *hip_stream), (B, L, zmp_x_tm, zmp_y_tm, state, com_tm, zmp2_tm, simulation, hip_stream)) \
  X(int, wg_preview_follow_dev, (int B, int lcap, const int *length, int *done, const double *zmp_x_tm, const double *zmp_y_tm, double *state, \
    double *com_tm, double *zmp2_tm, int simulation, void *hip_stream), (B, lcap, length, done, zmp_x_tm, zmp_y_tm, state, com_tm, zmp2_tm, simulation, \
    hip_stream)) \
  X(int, wg_preview_run_batch, (int B, int L, const double *zmp_x, const double *zmp_y, double *state, double *com, double *zmp2, int simulation), (B, L, \
    zmp_x, zmp_y, state, com, zmp2, simulation)) \
  X(int, wg_gramian_batch_dev, (int B, int N, const double *T, const double *h, double alpha, double beta, double gamma, int precision, double *Qb, \
    void *hip_stream), (B, N, T, h, alpha, beta, gamma, precision, Qb, hip_stream)) \
  X(int, wg_gramian_batch, (int B, int N, const double *T, const double *h, double alpha, double beta, double gamma, int precision, double *Qb), (B, N, T, h, \
    alpha, beta, gamma, precision, Qb)) \
  X(int, wg_zmpdisc_batch_dev, (const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, \
    int lcap, double *zmp_x_tm, double *zmp_y_tm, int *length, void *hip_stream), (model, B, smax, steps, n_steps, init_feet, lcap, zmp_x_tm, zmp_y_tm, \
    length, hip_stream)) \
  X(int, wg_zmpdisc_full_batch_dev, (const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, \
    double *right_tm, int *right_type_tm, int *length, void *hip_stream), (model, B, smax, steps, n_steps, init_feet, lcap, zmp_x_tm, zmp_y_tm, zmp_theta_tm, \
    zmp_type_tm, left_tm, left_type_tm, right_tm, right_type_tm, length, hip_stream)) \
  X(int, wg_zmpdisc_batch, (const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, \
    int lcap, double *zmp, double *zmp_theta, int *zmp_type, double *left, int *left_type, double *right, int *right_type, int *length), (model, B, smax, \
    steps, n_steps, init_feet, lcap, zmp, zmp_theta, zmp_type, left, left_type, right, right_type, length)) \
  X(int, wg_zmpdisc_begin_dev, (const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, \
    int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, \
    int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream), (model, B, smax, steps, n_steps, init_feet, lcap, zmp_x_tm, zmp_y_tm, \
    zmp_theta_tm, zmp_type_tm, left_tm, left_type_tm, right_tm, right_type_tm, state, length, hip_stream)) \
  X(int, wg_zmpdisc_append_dev, (const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, int lcap, \
    double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, \
    wg_zmpdisc_state_t *state, int *length, void *hip_stream), (model, B, smax, steps, n_steps, lcap, zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, \
    left_type_tm, right_tm, right_type_tm, state, length, hip_stream)) \
  X(int, wg_zmpdisc_end_dev, (const wg_zmpdisc_model_t *model, int B, const int *select, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, \
    int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream), \
    (model, B, select, lcap, zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, left_type_tm, right_tm, right_type_tm, state, length, hip_stream)) \
  X(int, wg_steps_plan_dev, (int B, int ccap, const wg_step_cmd_t *cmds, const int *n_cmds, double ss, double ds, wg_step_stack_t *stack, int smax, \
    wg_rel_step_t *steps, int *n_steps, void *hip_stream), (B, ccap, cmds, n_cmds, ss, ds, stack, smax, steps, n_steps, hip_stream)) \
  X(int, wg_mpc_blocks_batch_dev, (int M, const wg_model_t *models, void *blocks, int *status, void *hip_stream), (M, models, blocks, status, hip_stream)) \
  X(int, wg_mpc_blocks_batch, (int M, const wg_model_t *models, void *blocks, int *status), (M, models, blocks, status)) \
  X(int, wg_mpc_tick_fleet_dev, (int B, const wg_mpc_fleet_t *fleet, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls, int *hist, \
    int hist_cap, int *hist_len, void *hip_stream), (B, fleet, states, outs, diag, advance_calls, hist, hist_cap, hist_len, hip_stream)) \
  X(int, wg_mpc_run_fleet_dev, (int B, const wg_mpc_fleet_t *fleet, wg_gait_state_t *states, int n_ticks, int advance_calls, const double *vref_sched, \
    int period, wg_tick_out_t *outs, int *diag, void *hip_stream), (B, fleet, states, n_ticks, advance_calls, vref_sched, period, outs, diag, hip_stream)) \
  X(int, wg_zmpdisc_full_fleet_dev, (const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, \
    double *right_tm, int *right_type_tm, int *length, void *hip_stream), (fleet, B, smax, steps, n_steps, init_feet, lcap, zmp_x_tm, zmp_y_tm, zmp_theta_tm, \
    zmp_type_tm, left_tm, left_type_tm, right_tm, right_type_tm, length, hip_stream)) \
  X(int, wg_zmpdisc_begin_fleet_dev, (const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, \
    double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream), (fleet, B, smax, steps, n_steps, init_feet, lcap, \
    zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, left_type_tm, right_tm, right_type_tm, state, length, hip_stream)) \
  X(int, wg_zmpdisc_append_fleet_dev, (const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, int lcap, \
    double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, \
    wg_zmpdisc_state_t *state, int *length, void *hip_stream), (fleet, B, smax, steps, n_steps, lcap, zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, \
    left_type_tm, right_tm, right_type_tm, state, length, hip_stream)) \
  X(int, wg_zmpdisc_end_fleet_dev, (const wg_zmpdisc_fleet_t *fleet, int B, const int *select, int lcap, double *zmp_x_tm, double *zmp_y_tm, \
    double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, \
    void *hip_stream), (fleet, B, select, lcap, zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, left_type_tm, right_tm, right_type_tm, state, length, \
    hip_stream)) \
  X(int, wg_steps_plan_fleet_dev, (int B, int ccap, const wg_step_cmd_t *cmds, const int *n_cmds, const double *ss, const double *ds, wg_step_stack_t *stack, \
    int smax, wg_rel_step_t *steps, int *n_steps, void *hip_stream), (B, ccap, cmds, n_cmds, ss, ds, stack, smax, steps, n_steps, hip_stream)) \
  X(int, wg_foot_constraints_fleet_dev, (int B, int lcap, const int *length, const double *time, const double *left_tm, const int *left_type_tm, \
    const double *right_tm, const wg_sole_t *soles, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream), (B, \
    lcap, length, time, left_tm, left_type_tm, right_tm, soles, qcap, queues, t_start, t_end, count, hip_stream)) \
  X(int, wg_foot_constraints_append_fleet_dev, (int B, int lcap, int first_sample, int *done, const int *length, const double *time, const double *left_tm, \
    const int *left_type_tm, const double *right_tm, const wg_sole_t *soles, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, \
    void *hip_stream), (B, lcap, first_sample, done, length, time, left_tm, left_type_tm, right_tm, soles, qcap, queues, t_start, t_end, count, hip_stream)) \
  X(int, wg_zmp_audit_dev, (int B, int lcap, const int *length, const double *time, const double *px_tm, const double *py_tm, long long pitch, int qcap, \
    const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, wg_zmp_audit_t *audit, double *margin_tm, \
    void *hip_stream), (B, lcap, length, time, px_tm, py_tm, pitch, qcap, queues, t_start, t_end, count, audit, margin_tm, hip_stream)) \
  X(int, wg_zmp_audit_append_dev, (int B, int lcap, int first_sample, int *done, const int *length, const double *time, const double *px_tm, \
    const double *py_tm, long long pitch, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, \
    wg_zmp_audit_t *audit, double *margin_tm, void *hip_stream), (B, lcap, first_sample, done, length, time, px_tm, py_tm, pitch, qcap, queues, t_start, \
    t_end, count, audit, margin_tm, hip_stream)) \
  X(int, wg_morisawa_solve_dev, (const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, \
    const double *com0, void *blocks, int *status, void *hip_stream), (model, B, smax, steps, n_steps, init_feet, com0, blocks, status, hip_stream)) \
  X(int, wg_morisawa_solve_fleet_dev, (const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream), (models, B, smax, steps, n_steps, init_feet, com0, blocks, \
    status, hip_stream)) \
  X(int, wg_morisawa_sample_dev, (int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap, double *zmp_x_tm, \
    double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream), (B, smax, \
    blocks, status, t_start, T, lcap, zmp_x_tm, zmp_y_tm, com_tm, left_tm, left_type_tm, right_tm, right_type_tm, length, hip_stream)) \
  X(int, wg_morisawa_walk_dev, (const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, \
    const double *com0, void *blocks, int *status, double t_start, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, \
    int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream), (model, B, smax, steps, n_steps, init_feet, com0, blocks, \
    status, t_start, lcap, zmp_x_tm, zmp_y_tm, com_tm, left_tm, left_type_tm, right_tm, right_type_tm, length, hip_stream)) \
  X(int, wg_morisawa_walk_fleet_dev, (const wg_morisawa_model_t *models, double T, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, const double *com0, void *blocks, int *status, double t_start, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, \
    double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream), (models, T, B, smax, steps, n_steps, init_feet, \
    com0, blocks, status, t_start, lcap, zmp_x_tm, zmp_y_tm, com_tm, left_tm, left_type_tm, right_tm, right_type_tm, length, hip_stream)) \
  X(int, wg_morisawa_long_solve_dev, (const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream), (model, B, smax, steps, n_steps, init_feet, com0, blocks, \
    status, hip_stream)) \
  X(int, wg_morisawa_long_solve_fleet_dev, (const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream), (models, B, smax, steps, n_steps, init_feet, com0, blocks, \
    status, hip_stream)) \
  X(int, wg_morisawa_long_sample_dev, (int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap, double *zmp_x_tm, \
    double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream), (B, smax, \
    blocks, status, t_start, T, lcap, zmp_x_tm, zmp_y_tm, com_tm, left_tm, left_type_tm, right_tm, right_type_tm, length, hip_stream)) \
  X(int, wg_morisawa_long_walk_dev, (const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, const double *com0, void *blocks, int *status, double t_start, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, \
    double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream), (model, B, smax, steps, n_steps, init_feet, \
    com0, blocks, status, t_start, lcap, zmp_x_tm, zmp_y_tm, com_tm, left_tm, left_type_tm, right_tm, right_type_tm, length, hip_stream)) \
  X(int, wg_morisawa_long_walk_fleet_dev, (const wg_morisawa_model_t *models, double T, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, \
    const double *init_feet, const double *com0, void *blocks, int *status, double t_start, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, \
    double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream), (models, T, B, smax, steps, n_steps, init_feet, \
    com0, blocks, status, t_start, lcap, zmp_x_tm, zmp_y_tm, com_tm, left_tm, left_type_tm, right_tm, right_type_tm, length, hip_stream)) \
  X(int, wg_morisawa_resolve_dev, (const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors, const int *factor_of, \
    const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream), (model, B, smax, factors, \
    n_factors, factor_of, steps, init_feet, com0, blocks, status, hip_stream)) \
  X(int, wg_morisawa_resolve_fleet_dev, (const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors, const int *factor_of, \
    const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream), (models, B, smax, factors, \
    n_factors, factor_of, steps, init_feet, com0, blocks, status, hip_stream)) \
  X(int, wg_morisawa_long_resolve_dev, (const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors, const int *factor_of, \
    const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream), (model, B, smax, factors, \
    n_factors, factor_of, steps, init_feet, com0, blocks, status, hip_stream)) \
  X(int, wg_morisawa_long_resolve_fleet_dev, (const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors, \
    const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream), (models, \
    B, smax, factors, n_factors, factor_of, steps, init_feet, com0, blocks, status, hip_stream))
#define WG_CTX_UNPAREN_(...) __VA_ARGS__
#define WG_CTX_PROTO_(ret, name, params, args) ret name##_ctx(wg_ctx_t *ctx, WG_CTX_UNPAREN_ params);
WG_CTX_FORWARDED(WG_CTX_PROTO_)

#ifdef __cplusplus
}
#endif
#endif /* WG_MPC_H */
