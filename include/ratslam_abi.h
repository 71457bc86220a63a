/*
 * ratslam_abi.h -- C ABI of libratslam_hip.so, the MI355X (gfx950) hot path of
 * pyratslam: the pose-cell network step and the view-template matcher.
 *
 * Plain C types only (pointers + sizes); every entry point returns an int
 * status (RS_OK == 0) and leaves a thread-local message in rs_last_error().
 * Host buffers are caller-owned and copied during the call; device memory is
 * owned by the handle.  A handle is not re-entrant: callers serialise calls on
 * one handle (the Python wrapper holds a per-handle lock); distinct handles may
 * be used from different threads concurrently (ros_simulate.py:103 vs :135).
 * Calls may return once their results have reached host memory, before the
 * device work they queued has retired: a fault or launch error in that work is
 * then returned (RS_ERR_HIP) by a later call on the same handle that waits for
 * its stream -- at the latest by rs_pc_destroy / rs_vt_destroy, which always
 * synchronise and report it after freeing the handle.
 *
 * What each entry point replaces in the reference (/root/reference/ratslam):
 *   rs_pc_create    PoseCellNetwork.__init__      posecell_network.py:24-48
 *                   + Convolution(...)/set_params convolution.py:11-91
 *   rs_pc_update    PoseCellNetwork.update        posecell_network.py:326-353
 *                   (conv_im x3 + host inhibition/normalisation/clamps/argmax,
 *                    convolution.py:404-511, posecell_network.py:336-351)
 *   rs_pc_update_odom / rs_pc_run_odom
 *                   update(v) / run() taking the odometry itself: path_integration's
 *                   control (posecell_network.py:252-308) computed in the library
 *   rs_pc_excite    update() steps 1-4 alone      posecell_network.py:336-345
 *   rs_pc_run       a loop of update() calls      simulate.py:31-34, ros_simulate.py:134-137
 *   rs_pc_inject    PoseCellNetwork.inject        posecell_network.py:322-324
 *   rs_pc_get_max   PoseCellNetwork.get_pc_max    posecell_network.py:317-319
 *   rs_pc_read/write  the .posecells ndarray      posecell_network.py:27, simulate.py:60,
 *                                                 ros_simulate.py:140,145
 *   rs_vt_create    ViewTemplates.__init__        view_templates.py:42-57 (device library)
 *   rs_vt_add       templates.append(...)         view_templates.py:68-70
 *   rs_vt_match     ViewTemplates.match           view_templates.py:63-75
 *                   (scores = ViewTemplate.match  view_templates.py:16-28)
 *   rs_vt_match_batch  a loop of ViewTemplates.match calls (exact sequential
 *                   semantics incl. in-batch appends), or a frozen-library scan
 *   rs_vt_match_stream  many frozen-library batches, one host synchronisation
 *   rs_vt_read      ViewTemplate.template         view_templates.py:11
 *   rs_vt_scores    ViewTemplate.match per pair   view_templates.py:16-28 (uint8, wrapping)
 *   rs_vt_offset_profile  the per-offset sums of ViewTemplate.match and which offset won,
 *                   view_templates.py:19-27 (the reference keeps only the minimum)
 *   rs_sad_scores   ViewTemplate.match per pair   view_templates.py:16-28 (float32/float64)
 *   rs_vtf_create   ViewTemplates.__init__ for float frames  view_templates.py:42-57
 *   rs_vtf_add / rs_vtf_append_staged  templates.append(...)  view_templates.py:68-70
 *   rs_vtf_read     ViewTemplate.template         view_templates.py:11
 *   rs_vtf_scores   ViewTemplate.match per pair   view_templates.py:16-28 (float, resident)
 *   rs_vtf_scan     the match_val list, its min and np.argmin  view_templates.py:65-67,73
 *                   (the threshold decision of :67 stays with the caller)
 *   rs_sad_plan_sum np.sum inside ViewTemplate.match  view_templates.py:24 (host, the
 *                   summation plan the float kernels execute)
 *   rs_vt_set_threshold  the `min(match_val) > match_threshold` rule, view_templates.py:67
 *   rs_vt_set_subsample / rs_vt_match_frames
 *                   input[self.mask].reshape(...) view_templates.py:48-57,64 (on device)
 *   rs_comm_*, rs_vt_attach_comm  (new) RCCL sharding of the library over GPUs
 *   rs_vo_create    SimpleVisualOdometer()        ros_simulate.py:5, 90 (the imported module
 *                   is absent from the reference; the arithmetic is defined below)
 *   rs_vo_run       vis_odom.update(im) per frame ros_simulate.py:119-122, the (vtrans, vrot)
 *                   deltas the main loop feeds to update_posecells, :163-165
 *   rs_vo_select    the shift choice inside update(), on the host alone
 *   rs_em_*         (new) ExperienceMap with the linking the reference leaves as a TODO,
 *                   experience_map.py:58; rs_em_relax_host is the same rule on the host alone
 */
#ifndef RATSLAM_ABI_H
#define RATSLAM_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (the Python wrapper maps them to exceptions) */
#define RS_OK           0
#define RS_ERR_ARG      1   /* ValueError   (bad size / index / parameter)          */
#define RS_ERR_TYPE     2   /* TypeError    (shape/dtype mismatch, convolution.py:578-611) */
#define RS_ERR_LUT_KEY  3   /* KeyError     (filter LUT miss, posecell_network.py:249) */
#define RS_ERR_HIP      4   /* RuntimeError (HIP runtime failure)                    */
#define RS_ERR_RCCL     5   /* RuntimeError (RCCL failure)                           */
#define RS_ERR_STATE    6   /* RuntimeError (handle misuse)                          */
#define RS_ERR_NOMEM    7   /* MemoryError                                           */
#define RS_ERR_CTL_RANGE 8  /* (internal) odometry outside the uploaded control tables;
                               nothing ran, the caller computes the control itself     */

#define RS_PREC_F32 0
#define RS_PREC_F64 1

#define RS_FILTER_LEN 7     /* PC_E_DIM, posecell_network.py:12; convolution.py:40 */

/* library version, e.g. 100 for 0.1.0 */
int rs_version(void);
/* thread-local description of the last error on this thread ("" if none) */
const char* rs_last_error(void);
/* number of visible HIP devices (0 if none / no driver) */
int rs_device_count(void);
/* device buffers for callers that keep inputs resident in HBM without a framework
 * (e.g. camera frames for rs_vt_match_frames); rs_dev_copy copies in any direction */
int rs_dev_malloc(int device, size_t bytes, void** ptr);
int rs_dev_free(void* ptr);
int rs_dev_copy(void* dst, const void* src, size_t bytes);
/* pinned, GPU-visible host memory (hipHostMalloc, mapped + coherent): the target of
 * rs_pc_read_pinned, so the .posecells readback needs no host-side copy */
int rs_host_alloc(size_t bytes, void** ptr);
int rs_host_free(void* ptr);

/* ------------------------------------------------------------------------ */
/* Pose-cell network                                                         */
/* ------------------------------------------------------------------------ */
typedef struct rs_pc rs_pc;

typedef struct rs_pc_params {
    int precision;              /* RS_PREC_F32 (default) or RS_PREC_F64          */
    double global_inhibition;   /* PC_GLOBAL_INHIB = 0.2 (posecell_network.py:15) */
    /* 3-D excitation kernel K = (ge x ge x ge - gi x gi x gi) * k_scale, the exact
     * rank-2 form of diff_gaussian(order=3) (posecell_network.py:97-113).
     * The excitation is the periodic correlation out[i] = sum_t g[t] * P[i + t - 3] along
     * each axis, t = 0 .. 6 (the reference's kernel `conv`, convolution.py:228-246): tap t
     * reads the cell t - 3 places further on, so reversed taps are another kernel. */
    double ge[RS_FILTER_LEN];
    double gi[RS_FILTER_LEN];
    double k_scale;             /* 1 / |sum(ge^3 - gi^3)|                         */
    /* table of 7x7 path-integration filters (posecell_network.py:47,50-59),
     * row-major [nfilters][7][7], F[x][y] with x along the first grid axis.
     * The path step of layer k, with F = table[fidx[k]], is
     *   out[i][j][k] = sum_{x,y} F[x][y] * P[(i + x - 3 + ox[k]) % X][(j + y - 3 + oy[k]) % Y][k]
     * (convolution.py:320-340), and the theta pass that follows it is the same
     * correlation with zf: out[k] = sum_t zf[t] * P[(k + t - 3) % TH].
     * A table of more than 8 filters needs Y <= 128 (only the "rows" step kernels read
     * a table that is not staged in LDS); on a wider grid rs_pc_create returns
     * RS_ERR_ARG */
    int nfilters;
    const double* xy_filters;
} rs_pc_params;

/* Per-step control computed on the host from the odometry exactly as
 * path_integration does (posecell_network.py:253-308):
 *   ox, oy [TH]  integer shifts of each theta layer       (:262-265)
 *   fidx   [TH]  index into the xy filter table per layer  (:249,271)
 *   zf     [7]   1-D theta filter                           (:304-309)
 * Batched forms are laid out step-major: ox[n*TH], oy[n*TH], fidx[n*TH], zf[n*7]. */

int rs_pc_create(int X, int Y, int TH, const rs_pc_params* params, int device, rs_pc** out);
int rs_pc_destroy(rs_pc* h);
int rs_pc_shape(const rs_pc* h, int* X, int* Y, int* TH);

/* one full update(); out_xyz = argmax cell (first in C order), as max_pc */
int rs_pc_update(rs_pc* h, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                 const double* zf, int32_t out_xyz[3]);
/* n consecutive updates with one host round trip; out_xyz[n*3] (may be NULL) */
int rs_pc_run(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
              const double* zf, int32_t* out_xyz);
/* Odometry -> control inside the library (posecell_network.py:252-308), so update()
 * costs one FFI call and no NumPy.  The wrapper uploads, once, the tables the NumPy
 * path evaluates with NumPy's own functions -- per-layer cos/sin of the heading
 * (:257-261), the LUT key -> filter row map (:249), and the 1-D theta filters for
 * origins zorig_min .. zorig_min+nz-1 (:304-308) -- and the library then applies
 * only correctly rounded IEEE operations (division, one product, rint, trunc,
 * floor, no contraction), so the control is bit-identical to filters.step_control.
 * rs_pc_update_odom: RS_ERR_LUT_KEY after running steps 1-4 (the reference's state
 * when :249 raises); RS_ERR_CTL_RANGE, with nothing run, when the theta origin is
 * outside the uploaded filters (the caller then computes the control itself).
 * rs_pc_run_odom: odom[n*2] = (vtrans, vrot) per step; on a LUT miss at step s it
 * runs steps < s, then steps 1-4 of s, sets *first_bad = s and returns
 * RS_ERR_LUT_KEY (else *first_bad = -1).  A batch of 1,024 steps or more forms its
 * control on up to 8 host threads before its first launch (the same values; the
 * first failing step decides, as in order). */
int rs_pc_set_odometry_tables(rs_pc* h, double vtrans_scale, double vrot_scale,
                              const double* cos_a, const double* sin_a, int key_min,
                              int nkeys, const int32_t* key_rows, int zorig_min, int nz,
                              const double* zf_table);
int rs_pc_update_odom(rs_pc* h, double vtrans, double vrot, int32_t out_xyz[3]);
/* the same control on the host alone (no handle, no device): n steps of odom[n*2]
 * -> ox/oy/fidx[n*TH], zf[n*7] and a status per step (RS_OK, RS_ERR_LUT_KEY,
 * RS_ERR_CTL_RANGE; outputs of a failed step are partial) */
int rs_pc_odom_control(int TH, double vtrans_scale, double vrot_scale, const double* cos_a,
                       const double* sin_a, int key_min, int nkeys, const int32_t* key_rows,
                       int zorig_min, int nz, const double* zf_table, int n, const double* odom,
                       int32_t* ox, int32_t* oy, int32_t* fidx, double* zf, int32_t* status);
int rs_pc_run_odom(rs_pc* h, int n, const double* odom, int32_t* out_xyz, int* first_bad);
/* rs_pc_update_odom followed, on the same stream and before its one host sync, by the
 * export of the new volume into pinned memory from rs_host_alloc (as
 * rs_pc_read_pinned): update() and the .posecells read the ROS node makes after every
 * step (ros_simulate.py:134-145) as one round trip.  On an error the volume export
 * may not have run. */
int rs_pc_update_odom_read(rs_pc* h, double vtrans, double vrot, int32_t out_xyz[3], double* pinned_xyth);
/* steps 1-4 of update() alone (excitation, global inhibition, normalisation):
 * the state the reference leaves behind when path_integration raises KeyError */
int rs_pc_excite(rs_pc* h);
/* posecells[x][y][th] += energy; queued on the handle's stream (returns without a
 * host sync), ordered before the next update / read / argmax */
int rs_pc_inject(rs_pc* h, double energy, int x, int y, int th);
int rs_pc_get_max(rs_pc* h, int32_t out_xyz[3]);
/* Sub-cell pose: the activity packet's circular centroid round the first maximum, the
 * estimate ratslam-python and OpenRatSLAM return where the reference's get_pc_max is a
 * placeholder (posecell_network.py:316-320).  The library returns six float64 sums per
 * step, (S_x, C_x, S_y, C_y, S_th, C_th), over the wrapped box of (2r+1)^3 cells round
 * the step's argmax cell, by the rule of csrc/pc_peak_rule.h (every operation correctly
 * rounded, in a fixed order); the caller forms pose_a = atan2(S_a, C_a) * N_a / 2pi mod N_a.
 * The sums belong to the stored state, which may carry one positive factor common to all
 * cells (the halo form keeps it unnormalised between steps): only atan2 of a pair is
 * defined.  Where the stored state is what rs_pc_write wrote they are exactly the rule's.
 *   rs_pc_set_peak_tables  r = cells_to_avg in 1 .. 3 with 2r+1 <= min(X, Y, TH) (else
 *                          RS_ERR_ARG, before any device call); sc_a[2 N_a]: the axis's
 *                          sin weights sin(2 pi c / N_a), c = 0 .. N_a-1, then its cos
 *                          weights, as the caller's own math library evaluates them.
 *                          The calls below return RS_ERR_STATE before it.
 *   rs_pc_get_peak         the stored state's argmax cell and its sums (settles a pending
 *                          halo state as rs_pc_get_max does); one host sync.
 *   rs_pc_update_odom_peak, rs_pc_run_odom_peaks, rs_pc_run_peaks
 *                          rs_pc_update_odom, rs_pc_run_odom and rs_pc_run with each
 *                          step's sums (out_sums[n*6]) computed on the device behind the
 *                          step; the same statuses, *first_bad and state as those calls,
 *                          and the sums of the steps before a failing one are valid.
 *                          They wait for the stream's completion, never for polled words.
 *   rs_pc_peak_host        the rule on the host alone (no handle, no device) for the box
 *                          round cell xyz of a float64 C-order (X, Y, TH) volume. */
int rs_pc_set_peak_tables(rs_pc* h, int r, const double* sc_x, const double* sc_y, const double* sc_th);
int rs_pc_get_peak(rs_pc* h, int32_t xyz[3], double sums[6]);
int rs_pc_update_odom_peak(rs_pc* h, double vtrans, double vrot, int32_t out_xyz[3], double sums[6]);
int rs_pc_run_odom_peaks(rs_pc* h, int n, const double* odom, int32_t* out_xyz, double* out_sums,
                         int* first_bad);
int rs_pc_run_peaks(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                    const double* zf, int32_t* out_xyz, double* out_sums);
int rs_pc_peak_host(int X, int Y, int TH, int r, const double* volume_xyth, const int32_t xyz[3],
                    const double* sc_x, const double* sc_y, const double* sc_th, double sums[6]);
/* Injections inside a batched run: the view-template feedback without a host round trip
 * per frame.  A run of n steps takes ni injections; injection i is (inj_step[i],
 * inj_energy[i], inj_loc[3i .. 3i+2]) with 0 <= inj_step[i] <= n, the steps non-decreasing
 * in i, and a location that is one of
 *   (x, y, th)                  an explicit cell inside the grid;
 *   (RS_PC_INJ_AT_PEAK, ., .)   the first maximum of the state as it stands when the
 *                               injection is applied (what rs_pc_get_max would return there);
 *   (RS_PC_INJ_SAME_AS, k, .)   k < i: the cell injection k of this call resolved to.
 * The call is defined as this sequence on the same handle:
 *   for s in 0 .. n-1:
 *       for each injection i with inj_step[i] == s, in order:  rs_pc_inject(energy_i, cell_i)
 *       rs_pc_update_odom(odom[s])
 *   for each injection i with inj_step[i] == n, in order:      rs_pc_inject(energy_i, cell_i)
 * and returns the same peaks (out_xyz[n*3]), every injection's resolved cell
 * (out_inj_xyz[ni*3]) and leaves a stored volume equal to that sequence's bit for bit, in
 * every step form and both precisions.  With out_sums (may be NULL; RS_ERR_STATE before
 * rs_pc_set_peak_tables) step s's six sums are taken from the state before any injection
 * with step s + 1.  One host sync: the call waits for the stream's completion.
 * A LUT miss at step s (RS_ERR_LUT_KEY, *first_bad = s): the injections with
 * inj_step[i] <= s have been applied, the later ones have not and their cells come back as
 * (-1, -1, -1), and the state is the one the sequence leaves when its update fails.
 * RS_ERR_ARG before any device work, the state untouched: steps out of order, a step
 * outside [0, n], an explicit cell outside the grid, a same-as k >= i.  n == 0 with ni > 0
 * applies the injections alone.  The energy is not restricted (a NaN makes a NaN state).
 * rs_pc_run_inject: the same with the caller's control, as rs_pc_run is to rs_pc_run_odom. */
#define RS_PC_INJ_AT_PEAK (-1)   /* inj_loc[3i] */
#define RS_PC_INJ_SAME_AS (-2)   /* inj_loc[3i], inj_loc[3i+1] = k */
int rs_pc_run_odom_inject(rs_pc* h, int n, const double* odom, int ni, const int32_t* inj_step,
                          const double* inj_energy, const int32_t* inj_loc, int32_t* out_xyz,
                          int32_t* out_inj_xyz, double* out_sums, int* first_bad);
int rs_pc_run_inject(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                     const double* zf, int ni, const int32_t* inj_step, const double* inj_energy,
                     const int32_t* inj_loc, int32_t* out_xyz, int32_t* out_inj_xyz, double* out_sums);
/* whole volume as float64, C order (X, Y, TH) -- the reference's .posecells */
int rs_pc_read(rs_pc* h, double* host_xyth);
/* the same volume written by the GPU straight into pinned host memory from
 * rs_host_alloc (at least X*Y*TH doubles): one launch and a sync, no host copy --
 * the drop-in .posecells readback the ROS node pays every step (ros_simulate.py:140,145) */
int rs_pc_read_pinned(rs_pc* h, double* pinned_xyth);
int rs_pc_write(rs_pc* h, const double* host_xyth);
/* sum of all cells (float64 accumulation) */
int rs_pc_total(rs_pc* h, double* total);
/* device time of the last rs_pc_run/rs_pc_update, milliseconds (HIP events around
 * the step's launches; recorded only while profiling is enabled, else 0 -- the two
 * event records cost about 1.5 us of a 31 us update() call) */
int rs_pc_last_ms(rs_pc* h, double* ms);
/* profiling: enable = 1 records HIP events around the whole call (rs_pc_last_ms)
 * and around every launch (rs_pc_kernel_ms; the per-launch events add gaps between
 * the kernels); enable = 2 only around the whole call; 0 none.
 * rs_pc_kernel_ms: the event time of each kernel of the last rs_pc_run, summed over its
 * steps: ms[0] = the step kernel (excitation kernel of the two-launch forms, the one
 * kernel of the halo form), ms[1] = path-integration kernel (halo form: pc_halo_finish) */
int rs_pc_set_profiling(rs_pc* h, int enable);
int rs_pc_kernel_ms(rs_pc* h, double ms[2]);
/* step kernels in use: "rows" (row-tiled excite + path launches, Y <= 128),
 * "cols" (column tiles through all layers, large grids), "halo" (one launch per
 * step, the excitation recomputed on each tile's halo; float32, TH = 36, 18 or 10) or
 * "stream" (layer streaming, large grids outside the column form's limits) */
const char* rs_pc_step_form(const rs_pc* h);
/* Test hooks (no reference counterpart):
 *   RS_PC_DBG_POISON       fill every buffer a step writes before it reads (the
 *                          excited volume, the normalisation partials, the argmax
 *                          slots and partials, the host result words) with all
 *                          bits set, so that a read of anything the step did not
 *                          write shows up as NaN state or a wrong peak;
 *   RS_PC_DBG_SKIP_EXPORT  the next update/run leaves the host result words
 *                          unwritten: the call must fail with RS_ERR_HIP (the
 *                          check that every step's argmax reached the host);
 *   RS_PC_DBG_HALO_SETTLE  (halo form) every later call ends with the state
 *                          normalised by the finishing pass instead of left
 *                          unnormalised for the next call (A/B of the two paths);
 *   RS_PC_DBG_HALO_AMBIG   (rs_pc_debug_value) how many calls had their last step
 *                          keyed by the finishing pass because a cell lay within a
 *                          relative 2^-20 of the peak (pc_halo_export's RES_AMBIG). */
#define RS_PC_DBG_POISON      1
#define RS_PC_DBG_SKIP_EXPORT 2
#define RS_PC_DBG_HALO_SETTLE 3
#define RS_PC_DBG_HALO_AMBIG  4
int rs_pc_debug(rs_pc* h, int op);
int rs_pc_debug_value(rs_pc* h, int op, int64_t* value);

/* ------------------------------------------------------------------------ */
/* View templates                                                            */
/* ------------------------------------------------------------------------ */
typedef struct rs_vt rs_vt;

/* H x W uint8 templates, row shift max_offset (ViewTemplate.max_offset = 8,
 * view_templates.py:14), strict threshold match_threshold (:67).
 * capacity = initial number of templates this rank can hold (grows by doubling). */
int rs_vt_create(int H, int W, int max_offset, uint64_t match_threshold, int64_t capacity,
                 int device, rs_vt** out);
/* The metric of a uint8 library, fixed at create.
 *   RS_VT_METRIC_WRAPPED  sum of (T - Q) mod 256 per byte pair: numpy's own arithmetic on
 *                         uint8 arrays (the reference on mono8 frames); a pixel where the
 *                         query is one grey level above the template scores 255
 *   RS_VT_METRIC_SAD      sum of |T - Q| on the bytes as integers: the reference's
 *                         ViewTemplate.match on the same arrays cast to float
 * Everything behind a score -- packed keys, first argmin, threshold, in-batch candidates,
 * append, the min-reduction over ranks, rs_vt_match_stream / _frames / _scores -- is the
 * same for both.  rs_vt_create is rs_vt_create_metric with RS_VT_METRIC_WRAPPED.  Another
 * metric: RS_ERR_ARG before any device work, *out left NULL.  A SAD handle has no bit
 * planes and never prunes: RS_VT_SCAN, RS_VT_PRUNE and RS_VT_FRONT are not read for it. */
#define RS_VT_METRIC_WRAPPED 0
#define RS_VT_METRIC_SAD     1
int rs_vt_create_metric(int H, int W, int max_offset, uint64_t match_threshold, int64_t capacity,
                        int device, int metric, rs_vt** out);
int rs_vt_metric(const rs_vt* h, int* metric);
int rs_vt_destroy(rs_vt* h);
/* global number of stored templates (over all ranks) */
int rs_vt_count(const rs_vt* h, int64_t* count);
/* append n templates unconditionally (indices count .. count+n-1) */
int rs_vt_add(rs_vt* h, int n, const uint8_t* templates, int64_t* first_index);
/* read back template `index` (only on its owning rank: index % nranks == rank) */
int rs_vt_read(rs_vt* h, int64_t index, uint8_t* out);

#define RS_VT_FROZEN     0   /* score against the current library only, never append   */
#define RS_VT_SEQUENTIAL 1   /* exactly nq successive ViewTemplates.match calls          */

/* Match nq queries (each H x W uint8, already subsampled).  queries == NULL
 * re-matches the batch staged on the device by the previous call (same nq):
 * the queries stay resident in HBM across calls.
 * best_score[i]: the minimum score (UINT64_MAX if the library was empty)
 * best_index[i]: the index ViewTemplates.match returns (first argmin, or the
 *                new template's index when is_new[i] = 1)
 * is_new[i]:     1 if query i was appended as a new template                 */
int rs_vt_match_batch(rs_vt* h, int nq, const uint8_t* queries, int mode,
                      uint64_t* best_score, int64_t* best_index, uint8_t* is_new);
/* nb batches of nq queries each against the frozen library (nb successive
 * rs_vt_match_batch(RS_VT_FROZEN) calls), queued back to back on the device
 * with one host synchronisation.  queries[nb*nq*H*W]: host memory, or device
 * memory (rs_dev_malloc) whose batches the query-form kernels read in place.
 * Sharded handles reduce each batch with the RCCL allreduce(min) on the same
 * stream.  best_score / best_index[nb*nq] as in rs_vt_match_batch. */
int rs_vt_match_stream(rs_vt* h, int nb, int nq, const uint8_t* queries, uint64_t* best_score,
                       int64_t* best_index);
/* single query, RS_VT_SEQUENTIAL semantics */
int rs_vt_match(rs_vt* h, const uint8_t* query, uint64_t* best_score, int64_t* best_index,
                int* is_new);
/* On-device subsampling (view_templates.py:64, input[self.mask].reshape(shape)):
 * pixels[H*W] are the byte offsets, in a frame of frame_bytes, of the pixels the
 * mask keeps, in template row-major order (view_templates.py:48-57).  Then
 * rs_vt_match_frames matches nf whole frames (frame_bytes each; host memory, or
 * device memory the GPU gathers from in place) with rs_vt_match_batch semantics. */
int rs_vt_set_subsample(rs_vt* h, int64_t frame_bytes, const int32_t* pixels);
int rs_vt_match_frames(rs_vt* h, int nf, const uint8_t* frames, int mode, uint64_t* best_score,
                       int64_t* best_index, uint8_t* is_new);
/* all pair scores of nq queries vs templates [t0, t0+nt) (owning rank's slots only;
 * nranks must be 1): scores[q*nt + t]  -- ViewTemplate.match per pair */
int rs_vt_scores(rs_vt* h, int nq, const uint8_t* queries, int64_t t0, int64_t nt,
                 uint64_t* scores);
/* The row offset of a match (what OpenRatSLAM calls vt_relative_rad, in template rows): for
 * query i and template index[i], with M = max_offset,
 *   profile[i*(2M-1) + k] = sum_{r=M..H-M-1, c} term(T[r + k-(M-1)][c], Q[r][c]),  k = 0 .. 2M-2
 * (term by the handle's metric; min over k = the pair's score), and offset[i] = o of the
 * first minimal entry, o = k - (M-1): ViewTemplate.match's strict `<` from -M+1 upwards
 * (view_templates.py:19-27).  An empty window (H == 2M): zeros and offset -(M-1).
 * index[i] == -1: a row of UINT32_MAX and offset 0.  queries: nq*H*W host bytes, or device
 * memory read in place, or NULL for the batch the last rs_vt_match_batch / _frames / _match
 * staged (nq must be its size: RS_ERR_STATE otherwise) -- after a sequential match, a query
 * that matched a template appended earlier in its batch is profiled against that template.
 * Explicit queries leave the staged batch as it is.  profile may be NULL.  Any other index:
 * RS_ERR_ARG before any device work; a sharded handle: RS_ERR_STATE.  The call returns with
 * the results in the caller's arrays; its buffers are allocated by the first call.
 * rs_vt_offset_profile_host is the same rule for one raw H x W pair on the host alone (no
 * handle, no device). */
int rs_vt_offset_profile(rs_vt* h, int nq, const uint8_t* queries, const int64_t* index,
                         uint32_t* profile, int32_t* offset);
int rs_vt_offset_profile_host(int metric, int H, int W, int max_offset, const uint8_t* tpl,
                              const uint8_t* query, uint32_t* profile, int32_t* offset);
/* Patch normalisation (against a change of exposure between visits): with radius R > 0 every
 * raw image that enters the handle -- template, query, gathered frame, stream batch, explicit
 * offset-profile query -- is replaced on the device by its normalised bytes before anything
 * else reads it, so the library, every scan, rs_vt_read and rs_vt_offset_profile work on
 * normalised bytes.  At pixel (r, c), over the window of rows r-R..r+R and columns c-R..c+R
 * clamped to the image (n pixels, sum S, square sum S2):
 *   D = n*S2 - S*S,  N = n*p - S,  s = floor(sqrt(D)),
 *   out = 128 if s == 0, else clamp(128 + sign(N) * ((gain*|N| + s/2) / s), 0, 255)
 * in integers throughout (gain grey levels per local standard deviation around 128).
 * radius 0 turns it off (the default; gain is then ignored); a radius outside [0, 7] or a gain
 * outside [1, 127]: RS_ERR_ARG.  Allowed only while the handle holds no template and no staged
 * batch (RS_ERR_STATE otherwise), so a library never mixes raw and normalised bytes.  Device
 * and pinned inputs are read, never written.  Every rank of a sharded library sets the same.
 * rs_vt_normalise reads the setting back (0, 0 when off; either pointer may be NULL).
 * rs_vt_normalise_host is the same rule for one H x W image on the host alone (no handle, no
 * device): src and dst are distinct arrays of H*W bytes, radius in [1, 7]. */
int rs_vt_set_normalise(rs_vt* h, int radius, int gain);
int rs_vt_normalise(const rs_vt* h, int* radius, int* gain);
int rs_vt_normalise_host(int H, int W, int radius, int gain, const uint8_t* src, uint8_t* dst);
/* The two halves of rs_vt_match_batch, for callers that combine the per-rank
 * keys themselves (any min-reduction over ranks; key = score << 32 | index,
 * UINT64_MAX = no template):
 *   rs_vt_scan_local  stages the queries and returns this rank's keys;
 *   rs_vt_resolve     takes the global (min over ranks) keys of the staged
 *                     queries and applies ViewTemplates.match semantics,
 *                     appending the new templates this rank owns.            */
int rs_vt_scan_local(rs_vt* h, int nq, const uint8_t* queries, uint64_t* local_keys);
int rs_vt_resolve(rs_vt* h, int nq, const uint64_t* global_keys, int mode, uint64_t* best_score,
                  int64_t* best_index, uint8_t* is_new);
/* device time (ms) of the scan kernel in the last match call (HIP events): for
 * rs_vt_match_stream over HBM-resident batches, its one scan of all batches;
 * -1 when that scan ran untimed or the call ran several scans */
int rs_vt_last_ms(rs_vt* h, double* ms);
/* HIP events around every scan (default off).  Off, a match call's keys are polled in
 * pinned host memory (a plane scan's last block exports them itself) instead of a
 * stream synchronisation; on, two stream markers bracket each scan and the call
 * synchronises (rs_vt_last_ms) */
int rs_vt_set_timing(rs_vt* h, int enable);
/* which scan kernel family the handle uses for its shape: "plane" (bit-plane
 * borrow count, W == 32, H in {32, 64}, max_offset 8), "carry" (byte-SWAR carry
 * count, max_offset 8, H in {32, 64}; RS_VT_SCAN=carry forces it) or "generic";
 * NULL for a null handle.  "carry" names the family, not the launch: a key scan of
 * little work (fewer than 2,048 template blocks x queries, at most 8 dword columns)
 * runs its column form, vt_scan_carry_col_kernel; score matrices and every other
 * key scan run vt_scan_carry_kernel.  A RS_VT_METRIC_SAD handle: "sad" (max_offset 8,
 * H in {32, 64}, any W: a template column's rows in registers, v_sad_u8 per dword pair
 * and offset) or "sad-generic" (any other shape) */
const char* rs_vt_scan_form(const rs_vt* h);
/* "plane-pruned": a plane handle (H == 64) whose large frozen key scans prune template
 * blocks by an exact partial-score bound: a prefilter bounds every
 * (64-template block, query) pair from below, pass B1 scans each query against its
 * most promising block, pass B2 against every other block whose bound does not exceed
 * the score B1 found.  Before B1 the one template that holds the block's minimum bound
 * is scored exactly; where every other template's bound in the block exceeds that score
 * the query is settled without a block scan.  Ahead of such a scan
 * only the query planes of the aligned start rows are built; the verification expands
 * the rest for the queries a scan pass reads.  Exact for every
 * input.  RS_VT_PRUNE (read at create): "0"
 * dense launch everywhere ("plane"), "1" (default) prune scans of at least 512 queries
 * over at least two template blocks, "force" prune at any size.
 * rs_vt_prune_stats: of the last pruned scan launch, out[0] = the queries pass B1
 * settled in their candidate block, by verifying one template or by scanning the block
 * (= queries), out[1] = (block, query) pairs of pass B2, out[2] = template blocks x
 * queries, out[3] = scan passes launched; all 0 before the first pruned scan.  Reads the
 * device counters on demand (synchronises the handle's stream); the match calls do not.
 * RS_VT_PASSES (read at create): "1" (default) the verification writes one list per template
 * block on its verified score U0 >= U(q), a superset of the two passes' lists, and ONE list
 * pass scans it; "2" passes B1 and B2.  The statistics are the two-pass
 * rule's counts in either mode (out[3] == 2): with one pass a counting kernel takes them
 * on demand from what the call left. */
int rs_vt_prune_stats(rs_vt* h, int64_t out[4]);
/* *out = the (block, query) pairs the last pruned scan launch actually scanned: the entries
 * of its lists (with one pass the lists on U0: at least the two-pass rule's pairs plus the
 * unsettled queries); 0 before the first pruned scan.  Reads on demand like rs_vt_prune_stats. */
int rs_vt_prune_scanned(rs_vt* h, int64_t* out);
/* *out = the queries the last pruned scan launch settled by verification alone (they
 * took no block scan in pass B1); 0 before the first pruned scan.  Reads on demand like
 * rs_vt_prune_stats. */
int rs_vt_prune_verified(rs_vt* h, int64_t* out);

/* ViewTemplates.match's strict threshold (view_templates.py:67) as a double: a
 * score makes a new template when (double)score > threshold -- numpy's own
 * comparison of a uint64 score with a Python float (inf: never once the library
 * is non-empty; negative: always; NaN: never).  rs_vt_create's integer threshold
 * is the same rule for thresholds that are integers. */
int rs_vt_set_threshold(rs_vt* h, double threshold);

/* ViewTemplate.match on float arrays (view_templates.py:16-28 with float32 or
 * float64 data: no uint8 wrap, a true sum |T - Q| per row offset in the arrays'
 * precision, first strict minimum over the 2*max_offset-1 offsets from +inf).
 * The summation is np.sum's, bit for bit: numpy's pairwise order within each chunk of
 * 8,192 elements (its reduction buffer), the chunks' sums added in sequence; it is the
 * plan of the device-resident library below, which this call creates, fills and
 * destroys.  templates[nt*H*W], queries[nq*H*W] and scores[nq*nt] (scores[q*nt + t])
 * are host arrays of dtype RS_DT_F32 / F64 (another value: RS_ERR_TYPE); the scores are
 * computed on `device`.  Accepted, as by that library: H > 2*max_offset, W >= 1,
 * 1 <= max_offset <= 16, H*W <= 2^30, nt < 2^31, and a launch of at most 65,535 query
 * chunks (it splits the queries into no more than about 1,024 / nt); otherwise RS_ERR_ARG.
 * Zero nt or nq: RS_OK, nothing read or written. */
#define RS_DT_F32 0
#define RS_DT_F64 1
int rs_sad_scores(int device, int dtype, int H, int W, int max_offset, int64_t nt,
                  const void* templates, int nq, const void* queries, void* scores);

/* ------------------------------------------------------------------------ */
/* Device-resident float view-template library                               */
/* ------------------------------------------------------------------------ */
/* The float arithmetic of rs_sad_scores against a library that stays in HBM: a
 * camera pipeline whose frames are float32 / float64 (normalised to [0, 1], say)
 * uploads a template once and each match uploads only its queries.  Scores are
 * bit-identical to numpy's: the host lowers numpy's pairwise summation of the
 * (H - 2*max_offset) * W window into a plan (leaves of <= 128 elements with 8
 * strided accumulator chains, the fixed combine ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
 * the sequential tail, the postfix tree over the leaves) and the scan kernel runs
 * one chain per lane, combining by cross-lane exchange in the plan's order.
 * All templates, queries and scores of a handle have its dtype (RS_DT_F32 / F64;
 * another value: RS_ERR_TYPE); any H > 2*max_offset, W >= 1, 1 <= max_offset <= 16. */
typedef struct rs_vtf rs_vtf;

/* ViewTemplates.__init__ (view_templates.py:42-57) for float frames: an empty library
 * of H x W templates on `device`; capacity = initial slots (grows by doubling) */
int rs_vtf_create(int H, int W, int max_offset, int dtype, int64_t capacity, int device,
                  rs_vtf** out);
int rs_vtf_destroy(rs_vtf* h);
int rs_vtf_count(const rs_vtf* h, int64_t* count);
/* templates.append(...) (view_templates.py:68-70), unconditionally, n host templates */
int rs_vtf_add(rs_vtf* h, int n, const void* templates, int64_t* first_index);
/* ViewTemplate.template (view_templates.py:11): template `index` back to the host */
int rs_vtf_read(rs_vtf* h, int64_t index, void* out);
/* ViewTemplate.match per pair (view_templates.py:16-28): nq host queries against
 * templates [t0, t0+nt), scores[q*nt + t] as rs_vt_scores */
int rs_vtf_scores(rs_vtf* h, int nq, const void* queries, int64_t t0, int64_t nt, void* scores);
/* The scan of ViewTemplates.match (view_templates.py:65-67,73) for nq host queries
 * against the library as it stands (nothing is appended): best_score[i] = the
 * minimum of query i's match_val list, best_index[i] = np.argmin of it (the first
 * minimum); +inf / -1 for an empty library.  A score is never NaN (a NaN sum is
 * never taken, as `diff < mindiff` never takes it): an all-NaN pair scores +inf.
 * want_inbatch != 0 also fills inbatch[i*nq + j] for j < i with the score of staged
 * query i against staged query j as the template (not symmetric; entries with
 * j >= i are +inf), which is what a caller needs to resolve a batch with the
 * semantics of successive ViewTemplates.match calls.  The queries stay staged on
 * the device for rs_vtf_append_staged. */
int rs_vtf_scan(rs_vtf* h, int nq, const void* queries, int want_inbatch, void* best_score,
                int64_t* best_index, void* inbatch);
/* templates.append(...) (view_templates.py:68-70) for staged queries which[0..n)
 * of the last rs_vtf_scan / rs_vtf_scores, in that order, device to device */
int rs_vtf_append_staged(rs_vtf* h, int n, const int32_t* which, int64_t* first_index);
/* HIP events around the scan and its argmin reduction (default off), and their time
 * for the last rs_vtf_scan in ms; -1 when it ran untimed or the library was empty */
int rs_vtf_set_timing(rs_vtf* h, int enable);
int rs_vtf_last_ms(rs_vtf* h, double* ms);
/* np.sum of view_templates.py:24 on the host alone (no handle, no device): the sum
 * of values[0..n) of dtype RS_DT_F32 / F64 evaluated through the very plan the scan
 * kernel executes for a window of n elements, lane for lane, in that precision.
 * Equal to numpy's np.sum bit for bit; checks the summation order without a GPU. */
int rs_sad_plan_sum(int dtype, int64_t n, const void* values, void* out);

/* ------------------------------------------------------------------------ */
/* Scanline visual odometer                                                  */
/* ------------------------------------------------------------------------ */
/* The odometer of the node's camera-only mode (USE_VISUAL_ODOMETRY, ros_simulate.py:81:
 * no odometry subscription, every frame through vis_odom.update(im), :119-122).  The
 * reference fixes the interface only; the arithmetic, in exact integers:
 *   region   rows [y0, y1) x columns [x0, x1) of a mono8 frame, one for `trans`, one for
 *            `rot`;  R = y1 - y0, Wd = x1 - x0
 *   profile  prof[c] = sum over the region's rows of frame[y][x0 + c]          (uint32)
 *   table    against the previous frame's profile of the same region, for signed shifts
 *            s in [-(S-1), S-1]:  tab[s] = sum |cur[k] - prev[k + s]| over the Wd - |s|
 *            values of k with both indices valid (uint32, stored at index s + S - 1)
 *   select   best = +inf, shift = 0; for o = 0 .. S-1, candidates s = -o then s = +o:
 *            v = (double)tab[s] / (double)((Wd - o) * R * 255), taken if v < best
 *   deltas   vrot = shift_rot * rad_per_column;
 *            vtrans = min(best_trans * vtrans_scale, vtrans_max)
 * S = max_shift in [1, 64], Wd >= S and R * 255 * Wd < 2^32 per region, else RS_ERR_ARG
 * (checked before any device call).  A positive shift: new[k] == old[k + s].  The first
 * frame after rs_vo_create / rs_vo_reset returns (0, 0), has an all-zero table and only
 * stores its profiles; the state carries across calls. */
typedef struct rs_vo rs_vo;

typedef struct rs_vo_params {
    int trans_y0, trans_y1, trans_x0, trans_x1;
    int rot_y0, rot_y1, rot_x0, rot_x1;
    int max_shift;
    double rad_per_column;      /* radians(fov_deg) / im_w, computed by the caller */
    double vtrans_scale;
    double vtrans_max;
} rs_vo_params;

int rs_vo_create(int im_h, int im_w, const rs_vo_params* params, int device, rs_vo** out);
/* synchronises and reports an error of queued work, like rs_vt_destroy */
int rs_vo_destroy(rs_vo* h);
/* forget the previous frame: the next one returns (0, 0) */
int rs_vo_reset(rs_vo* h);
/* nf frames (im_h * im_w bytes each, back to back; host memory, staged 256 frames at a
 * time through pinned memory, or device memory read in place) -> deltas[nf*2] =
 * (vtrans, vrot) per frame.  Optional exports, both regions per frame, trans first:
 * tables[nf * 2 * (2*max_shift - 1)], profiles[nf * (Wd_trans + Wd_rot)] (NULL: none). */
int rs_vo_run(rs_vo* h, int nf, const uint8_t* frames, double* deltas, uint32_t* tables,
              uint32_t* profiles);
/* the selection rule on the host alone (no handle, no device): table[2*max_shift - 1] of
 * a region `width` columns by `rows` rows -> the shift and its normalised difference */
int rs_vo_select(int max_shift, int width, int rows, const uint32_t* table, int* shift,
                 double* mindiff);
/* HIP events around the profile and the shift launches (default off); rs_vo_last_ms:
 * ms[0] = profile kernel, ms[1] = shift kernel of the last rs_vo_run, -1 when it ran
 * untimed or in several chunks */
int rs_vo_set_timing(rs_vo* h, int enable);
int rs_vo_last_ms(rs_vo* h, double ms[2]);

/* ------------------------------------------------------------------------ */
/* Linked experience map                                                     */
/* ------------------------------------------------------------------------ */
/* The map the reference leaves at "TODO: linking will go here" (experience_map.py:58):
 * experiences with a pose (x, y, th), an append-only list of links l = (a -> b, d, h, f)
 * -- distance, heading and facing of b as measured from a -- and a damped-Jacobi
 * relaxation over the links.  All float64, correctly rounded, no contraction:
 *   wrap(t)  = t - 2pi * rint(t / 2pi)
 *   link     ex = x_b - (x_a + d * cos(th_a + h)), ey the same with sin,
 *            df = wrap(th_b - (th_a + f))
 *   sweep    (reads the previous iterate only) experience i sums from +0.0, in order, its
 *            links with i == a by ascending link id, each (+ex, +ey, +df), then its links
 *            with i == b by ascending link id, each (-ex, -ey, -df);  w = correction / deg_i;
 *            x' = x + w * sx;  y' = y + w * sy;  th' = wrap(th + w * st);
 *            an experience without links keeps its pose
 * The poses live on the device; the link list and the bookkeeping of which template owns
 * which experience stay with the caller (pyratslam_amd/linked_experience_map.py).
 * Kernel form: "lds" (one workgroup, both iterates in LDS, all sweeps in one launch) while
 * the map has at most 768 experiences, "sweep" (one launch per sweep over two global
 * buffers) above, each where it measured faster; both give the same bits.
 * RS_EM_FORM=lds|sweep, read at rs_em_create, forces one -- the lds form holds 3,072
 * experiences, and forced beyond that rs_em_relax returns RS_ERR_ARG. */
typedef struct rs_em rs_em;

/* capacity: experiences allocated at once (>= 1; the map grows by doubling);
 * correction in (0, 1] */
int rs_em_create(int capacity, double correction, int device, rs_em** out);
/* synchronises and reports an error of queued work, like rs_vt_destroy */
int rs_em_destroy(rs_em* h);
int rs_em_count(rs_em* h, int* nexp, int* nlinks);
/* a new experience reached from experience `from` by the measurement (d, heading, facing):
 * (x + d * cos(th + heading), y + d * sin(th + heading), wrap(th + facing)), computed on the
 * device from `from`'s current pose (queued); from == -1: the origin (0, 0, facing).  It
 * adds no link. */
int rs_em_add_experience(rs_em* h, int from, double d, double heading, double facing, int* id);
/* append the link from -> to; RS_ERR_ARG for ids out of range and for from == to */
int rs_em_add_link(rs_em* h, int from, int to, double d, double heading, double facing, int* id);
/* `loops` sweeps over all links, queued on the handle's stream: does not synchronise.  The
 * incidence lists are rebuilt on the host and uploaded only when experiences or links were
 * added since the last relax. */
int rs_em_relax(rs_em* h, int loops);
/* poses [first, first + n) as xyth[3 * n], after everything queued before */
int rs_em_read(rs_em* h, int first, int n, double* xyth);
int rs_em_write(rs_em* h, int first, int n, const double* xyth);
/* HIP events around the launches of every later rs_em_relax (default off); rs_em_last_ms
 * waits for the last relax and gives its device time, -1 when it ran untimed */
int rs_em_set_timing(rs_em* h, int enable);
int rs_em_last_ms(rs_em* h, double* ms);
/* "lds" or "sweep": the form rs_em_relax takes at the map's present size */
const char* rs_em_form(rs_em* h);
/* the same sweeps on the host alone (no handle, no device), through the library's own
 * incidence-list builder: nlinks links (from, to, d, heading, facing) over nexp experiences,
 * xyth[3 * nexp] relaxed in place */
int rs_em_relax_host(int nexp, int nlinks, const int32_t* from, const int32_t* to, const double* d,
                     const double* heading, const double* facing, double* xyth, int loops,
                     double correction);

/* ------------------------------------------------------------------------ */
/* Pose-cell ensemble                                                        */
/* ------------------------------------------------------------------------ */
/* B independent float32 pose-cell networks of one shape, each stepped by one workgroup out
 * of a compute unit's LDS.  A member's result depends on its own state
 * and control only: not on B, on its index, or on how a run is cut into launches.
 *   rs_pce_fit      host only: *lds_bytes (may be NULL) = the LDS a member's workgroup needs;
 *                   RS_ERR_ARG when a dimension is below 7 or the plan exceeds 160 KiB
 *   rs_pce_create   params as for rs_pc_create (precision must be RS_PREC_F32, at most 16
 *                   filters); global_inhibition[B], or NULL for params' value in every
 *                   member.  Volumes start all zero.  Argument errors (RS_ERR_ARG, *out NULL)
 *                   come before any device call.  RS_PCE_CHUNK=K in the environment forces
 *                   K steps per launch (default: what keeps a launch's control in 32 MiB).
 *   rs_pce_run      n steps of every member, one host synchronisation; member-major arrays
 *                   ox, oy, fidx [(m * n + s) * TH + k], zf [(m * n + s) * 7 + t] and
 *                   out_xyz [(m * n + s) * 3]: each step's first maximum in C order.  A null
 *                   array or a fidx outside the table: RS_ERR_ARG, nothing run.
 *   rs_pce_inject   posecells[member][x][y][th] += energy, member -1: every member; queued
 *   rs_pce_get_max  out_xyz[B * 3]: each member's first maximum in C order
 *   rs_pce_read, rs_pce_write   members [first, first + count) as float64, C order
 *                   (member, X, Y, TH); a value that is not a finite float32 is refused
 *                   (RS_ERR_ARG, nothing written)
 *   rs_pce_set_timing, rs_pce_last_ms   HIP events around the launches of every later
 *                   rs_pce_run or rs_pce_run_inject; the last run's device time in ms, -1 when
 *                   it ran untimed
 *
 * Injections and the sub-cell pose inside a run: rs_pc_run_inject's rule,
 * per member.
 *   rs_pce_set_peak_tables   as rs_pc_set_peak_tables: r in 1 .. 3 with 2r+1 <= min(X, Y, TH)
 *                   (else RS_ERR_ARG, before any device call), sc_a[2 N_a] the axis's sin then
 *                   cos weights.  The sums below return RS_ERR_STATE before it.
 *   rs_pce_get_peak out_xyz[B * 3], out_sums[B * 6]: each member's stored first maximum (as
 *                   rs_pce_get_max) and the six sums (S_x, C_x, S_y, C_y, S_th, C_th) of
 *                   csrc/pc_peak_rule.h over the box round it; one host synchronisation.
 *   rs_pce_run_inject   rs_pce_run with ni injections; injection i is (inj_member[i],
 *                   inj_step[i], inj_energy[i], inj_loc[3i .. 3i+2]) with 0 <= member < B,
 *                   0 <= step <= n, the steps non-decreasing within each member in list order
 *                   (the order across members is free), and a location that is one of
 *                     (x, y, th)                 an explicit cell inside the grid;
 *                     (RS_PC_INJ_AT_PEAK, ., .)  the first maximum in C order of that member's
 *                                                state as it stands when the injection is
 *                                                applied: what rs_pce_get_max would return there;
 *                     (RS_PC_INJ_SAME_AS, k, .)  k < i and inj_member[k] == inj_member[i]: the
 *                                                cell injection k resolved to.
 *                   The call is defined, for every member m, as this sequence:
 *                     for s in 0 .. n-1:
 *                         for each i of member m with inj_step[i] == s, in order:
 *                             rs_pce_inject(m, energy_i, cell_i)
 *                         one step of member m with step s's control
 *                     for each i of member m with inj_step[i] == n, in order:
 *                             rs_pce_inject(m, energy_i, cell_i)
 *                   and gives the peaks (out_xyz), the resolved cells (out_inj_xyz[ni * 3], in the
 *                   caller's order) and the stored volumes of that sequence made call by call,
 *                   bit for bit, whatever B, the member's place and the cut into launches.  An
 *                   injection is rs_pce_inject's float32 += of (float)energy.  With out_sums
 *                   (may be NULL; [(m * n + s) * 6]) step s's six sums are over the box round
 *                   step s's peak, of the state before any injection with step s + 1; the
 *                   ensemble stores the normalised state, so they are exactly the rule's, with
 *                   no common factor.  RS_ERR_ARG before any device work, the state untouched:
 *                   a member outside [0, B), steps out of order within a member, a step
 *                   outside [0, n], an explicit cell outside the grid, a same-as k >= i or of
 *                   another member, an energy that is not a finite float32.  n == 0 with
 *                   ni > 0 applies the injections alone.  With ni == 0 and out_sums NULL it is
 *                   rs_pce_run: the same launches, one host synchronisation either way. */
typedef struct rs_pce rs_pce;
int rs_pce_fit(int X, int Y, int TH, size_t* lds_bytes);
int rs_pce_create(int B, int X, int Y, int TH, const rs_pc_params* params,
                  const double* global_inhibition, int device, rs_pce** out);
int rs_pce_destroy(rs_pce* h);
int rs_pce_shape(const rs_pce* h, int* B, int* X, int* Y, int* TH);
int rs_pce_run(rs_pce* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
               const double* zf, int32_t* out_xyz);
int rs_pce_inject(rs_pce* h, int member, double energy, int x, int y, int th);
int rs_pce_get_max(rs_pce* h, int32_t* out_xyz);
int rs_pce_read(rs_pce* h, int first, int count, double* volumes);
int rs_pce_write(rs_pce* h, int first, int count, const double* volumes);
int rs_pce_set_timing(rs_pce* h, int enable);
int rs_pce_last_ms(rs_pce* h, double* ms);
int rs_pce_set_peak_tables(rs_pce* h, int r, const double* sc_x, const double* sc_y, const double* sc_th);
int rs_pce_get_peak(rs_pce* h, int32_t* out_xyz, double* out_sums);
int rs_pce_run_inject(rs_pce* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                      const double* zf, int ni, const int32_t* inj_member, const int32_t* inj_step,
                      const double* inj_energy, const int32_t* inj_loc, int32_t* out_xyz,
                      int32_t* out_inj_xyz, double* out_sums);

/* Multi-GPU: one process per GPU, library sharded round-robin (template g lives
 * on rank g % nranks at slot g / nranks); per query the local first-argmin keys
 * (score << 32 | g) are combined with one RCCL allreduce(min, uint64).        */
#define RS_UNIQUE_ID_BYTES 128
int rs_comm_unique_id(uint8_t id[RS_UNIQUE_ID_BYTES]);
int rs_vt_attach_comm(rs_vt* h, int rank, int nranks, const uint8_t id[RS_UNIQUE_ID_BYTES]);
/* shard without a communicator (the caller reduces keys between scan_local and resolve) */
int rs_vt_set_shard(rs_vt* h, int rank, int nranks);
int rs_vt_rank(const rs_vt* h, int* rank, int* nranks);

#ifdef __cplusplus
}
#endif
#endif /* RATSLAM_ABI_H */
