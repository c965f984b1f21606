/*
 * sdm_c.h -- C ABI of the MI355X semi-dense mapping engine (libsdm_hip.so).
 *
 * Drop-in boundary for the ProbabilityMapping hot path of atlas-jj/ORB-SLAM-free-space-carving.
 * The reference has no FFI/plugin registry for this path -- it is a plain C++ class
 * (/root/reference/include/Modeler/ProbabilityMapping.h:61-105, "PM.h").  Each entry point below
 * names the reference method it replaces; include/sdm/ProbabilityMapping.h keeps the reference's
 * class surface and forwards here.  Plain pointers and sizes only; no torch/HIP types.
 *
 * Conventions
 *  - "rho" is INVERSE depth (PM.cc:352-353: Z = 1/inv_d); maps are row-major, stride W.
 *  - keyframes live in numbered device slots [0, max_keyframes); all share W x H.
 *  - every call returns 0 on success or an SDM_E* code; sdm_last_error() has the text.  The
 *    reference's methods are void and unchecked (PM.cc passim); the C++ wrapper logs to cerr.
 *  - a context is single-caller (not re-entrant), like the reference's single mapping thread
 *    (PM.cc:65-87).  Work is queued on the context's HIP stream; host-pointer calls synchronise.
 *  - there is NO CPU fallback: without a visible gfx950 device sdm_create fails.
 */
#ifndef SDM_C_H
#define SDM_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDM_OK 0
#define SDM_EINVAL 1   /* bad argument (slot, size, null pointer, n > max_neighbours ...) */
#define SDM_EHIP 2     /* HIP runtime error (text in sdm_last_error) */
#define SDM_ENODEV 3   /* no usable GPU */
#define SDM_ESTATE 4   /* slot not uploaded / stage not run yet */
#define SDM_ECOMM 5    /* RCCL error or library not loadable (text in sdm_last_error) */

#define SDM_MAX_NEIGHBOURS 64
#define SDM_MAX_OBSERVATIONS 8192 /* keypoints / point depths per keyframe (sdm_upload_observations*) */

typedef struct sdm_ctx sdm_ctx;

/* PM.h:38-49 macros as runtime parameters (defaults = the reference's values). */
typedef struct {
    float lambdaG;     /* 8    PM.h:40  gradient gate (PM.cc:201,411,562)          */
    float lambdaL;     /* 80   PM.h:41  epipolar-line angle gate, deg (PM.cc:421)   */
    float lambdaTheta; /* 45   PM.h:42  orientation gate, deg (PM.cc:431)           */
    int lambdaN;       /* 3    PM.h:43  (PM.cc:221 '>', :623 '>=', :762 '<')        */
    double theta_var;  /* 0.23 PM.h:47  THETA, a double literal (PM.cc:436,455-456) */
} sdm_params;

typedef struct {
    int device;           /* HIP device ordinal */
    int W, H;             /* image size shared by all keyframes */
    int max_keyframes;    /* number of device slots */
    int max_neighbours;   /* <= SDM_MAX_NEIGHBOURS; reference covisN = 7 (PM.h:38) */
    int batch_capacity;   /* keyframes processed per launch group (scratch size); 0 = default */
    int with_pointset;    /* allocate the xyz pool (12 B/px/keyframe) for sdm_pointset */
    void *ext_depth_pool; /* optional caller-owned DEVICE buffer of sdm_depth_pool_bytes(); lets the
                             host framework (e.g. torch.distributed/RCCL) all-gather it in place */
    void *stream;         /* optional hipStream_t to run on (NULL = context-owned stream) */
} sdm_config;

typedef struct {
    long long searches;   /* EpipolarSearch invocations (pixel, neighbour)  PM.cc:213 */
    long long candidates; /* scan-loop iterations                           PM.cc:405 */
    long long gate_pass;  /* candidates that reached the cost               PM.cc:433 */
    long long hypotheses; /* accepted hypotheses                            PM.cc:216 */
    long long fused;      /* pixels written                                 PM.cc:225 */
    /* how K1 walked the ranges (not reference quantities): */
    long long mask_waves; /* (wave, neighbour) scans that took the gradient-mask scan instead of the batched one */
    long long mask_steps; /* mask words those scans examined (lane steps) */
    long long mask_row_mismatch; /* self-check of the mask scan's row runs: must stay 0 */
    long long open_pixels; /* fusing pixels neither shortcut of InverseDepthHypothesisFusion settled: all-pairs count, PM.cc:598-626 */
    long long table_stagings; /* host: compute calls whose slot / constant tables were not found in a cached set (K1 -> K4 -> K5
                                 of one step share one; counted whether or not statistics are enabled) */
} sdm_stats;

/* ---- lifetime ------------------------------------------------------------------------------- */
void sdm_default_params(sdm_params *p);
void sdm_default_config(sdm_config *c);
size_t sdm_depth_pool_bytes(int W, int H, int max_keyframes); /* = 8*W*H*max_keyframes */
int sdm_create(sdm_ctx **out, const sdm_config *cfg); /* replaces ProbabilityMapping(Map*) PM.cc:61 */
void sdm_destroy(sdm_ctx *ctx);
const char *sdm_last_error(void);
int sdm_set_params(sdm_ctx *ctx, const sdm_params *p);
int sdm_get_params(sdm_ctx *ctx, sdm_params *out); /* the parameters in force */
int sdm_set_stream(sdm_ctx *ctx, void *hip_stream);
int sdm_synchronize(sdm_ctx *ctx);
int sdm_device_count(void); /* number of visible HIP devices, 0 if none; never initialises a context */

/* ---- keyframe inputs (the KeyFrame members PM.cc reads) --------------------- */
/* im_: H*W u8; GradImg, GradTheta (degrees [0,360)): H*W f32; I_stddev; K = {fx,fy,cx,cy}
 * (include/KeyFrame.h:162); Tcw = world->camera [R|t] row-major 3x4 (src/KeyFrame.cc:70-121). */
int sdm_upload_keyframe(sdm_ctx *ctx, int slot, const uint8_t *im, const float *grad,
                        const float *theta, float I_stddev, const float K[4], const float Tcw[12]);
/* gray image only: GradImg/GradTheta/I_stddev computed on device (Scharr/32, magnitude,
 * fastAtan2 phase, population sigma) -- the pre-processing the reference leaves to the caller. */
int sdm_upload_image(sdm_ctx *ctx, int slot, const uint8_t *im, const float K[4],
                     const float Tcw[12]);
/* The step before the path: a camera frame as Tracking receives it.  Replaces, on the device,
 * Tracking::GrabImageMonocular's cvtColor(RGB/BGR/RGBA/BGRA -> GRAY) (src/Tracking.cc:244-257), the
 * cv::undistort(im, imu, mK, mDistCoef) of src/Tracking.cc:266-271 and the cvtColor(CV_RGB2GRAY) the Modeler applies
 * to the stored frame (src/Modeler/Modeler.cc:154-155): undistort the colour frame (1/32-pixel fixed-point map,
 * bilinear, zero border), convert to gray (4899/9617/1868 >> 14), then the gradient pre-pass of sdm_upload_image.
 * pixels: H*W interleaved pixels of 1, 3 or 4 bytes.  dist = {k1,k2,p1,p2,k3} as in Examples/Monocular/TUM1.yaml
 * (Camera.k1.. ; src/Tracking.cc:65-75), NULL = the frame is already undistorted.  The fork's Modeler converts
 * with CV_RGB2GRAY whatever Camera.RGB says: pass SDM_ORDER_RGB to reproduce that, the true order for a correct gray.
 * Bit-exact with OpenCV 2.4.5's cvUndistort2 + cvCvtColor and cvSobel(CV_SCHARR)/32 + cvCartToPolar
 * (tests/test_gpu_opencv_pin.py). */
#define SDM_ORDER_RGB 0
#define SDM_ORDER_BGR 1
#define SDM_ORDER_RGBA 2
#define SDM_ORDER_BGRA 3
#define SDM_ORDER_GRAY 4
int sdm_upload_image_rgb(sdm_ctx *ctx, int slot, const uint8_t *pixels, int order, const float K[4],
                         const float dist[5], const float Tcw[12]);
/* The same two calls for n keyframes at once (what Tracking / Modeler::AddFrameImage hand over,
 * src/Tracking.cc:244-271, src/Modeler/Modeler.cc:1496-1514, for a whole window of keyframes): ONE launch each of the
 * pre-pass kernels over (keyframe, tile) instead of a dozen launch-latency-sized ones per keyframe, H2D copies on an
 * upload stream overlapping the previous chunk's kernels.  images[i] / pixels[i]: host pointers; memory from
 * sdm_host_alloc (pinned) is read in place by the copy engine, any other memory is staged through a pinned ring.
 * K: [n][4], Tcw: [n][12]; dist (shared by the batch, as is K when dist != NULL) as above.  Every caller buffer is free
 * on return.  Results are bit-identical to n single calls (tests/test_gpu_ingest.py). */
int sdm_upload_images_batch(sdm_ctx *ctx, int n, const int *slots, const uint8_t *const *images,
                            const float *K, const float *Tcw);
int sdm_upload_images_rgb_batch(sdm_ctx *ctx, int n, const int *slots, const uint8_t *const *pixels,
                                int order, const float *K, const float dist[5], const float *Tcw);
/* pinned host memory for frame queues (the fork's Modeler keeps its own copies of the frames, Modeler.cc:1496-1514:
 * kept in memory from here they reach the device without a staging copy); NULL when the allocation fails */
void *sdm_host_alloc(size_t bytes);
void sdm_host_free(void *p);
/* same, image already resident in device memory */
int sdm_upload_image_device(sdm_ctx *ctx, int slot, const void *d_im, const float K[4],
                            const float Tcw[12]);
/* pose changed after bundle adjustment (kf->poseChanged, PM.cc:329) */
int sdm_set_pose(sdm_ctx *ctx, int slot, const float Tcw[12]);
/* read back what the device derived for a slot (for tests): any pointer may be NULL */
int sdm_download_inputs(sdm_ctx *ctx, int slot, uint8_t *im, float *grad, float *theta,
                        float *I_stddev);

/* ---- SemiDenseRecon, PM.h:75 / PM.cc:137-256, batched over n_ref reference keyframes --------- */
/* nbr_slots and rot_deg are [n_ref][n]; rot_deg may be NULL (= 0, "kf pair without
 * covisibility", PM.cc:174-177).  min_depth/max_depth are [n_ref], named as in PM.cc:381-382. */
int sdm_search_fuse(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n, const int *nbr_slots,
                    const float *rot_deg, const float *min_depth,
                    const float *max_depth);                            /* PM.cc:197-231 */
int sdm_intra_check(sdm_ctx *ctx, int n_ref, const int *ref_slots);     /* PM.cc:486-547 */
int sdm_intra_grow(sdm_ctx *ctx, int n_ref, const int *ref_slots);      /* PM.cc:549-596 */
int sdm_recon(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n, const int *nbr_slots,
              const float *rot_deg, const float *min_depth, const float *max_depth);

/* ---- search priors from the keyframes' ORB observations, on the device -------------------------
 * What SemiDenseRecon derives before its search: the median in-plane rotation of every (reference, neighbour) pair
 * (GetRotInPlane + median, PM.cc:170-179 and 467-484) and the inverse-depth bounds of every reference
 * (StereoSearchConstraints, PM.cc:184 and 370-383), equal to sdm_median_rot_in_plane (as floats, -0 == +0) and bitwise
 * equal to sdm_stereo_search_constraints.
 *
 * A slot holds its keyframe's observations as sdm::KeyFrame carries them: map_point_ids[n_kp] (< 0 = no map point),
 * angles[n_kp] (mvKeysUn[i].angle, degrees, < 0 = no angle), depths[n_depths] (GetAllPointDepths()).  Only entries with
 * id >= 0 && angle >= 0 are kept for the priors, sorted by id on the device; beside them the sorted id >= 0 list whatever
 * the angle, for the covisibility weights below.  Order: upload the slot's image FIRST -- every image upload
 * into a slot (sdm_upload_keyframe, sdm_upload_image*, the batch and device variants) marks its observations absent.
 * Memory: nothing until the first observation upload; then 16 * SDM_MAX_OBSERVATIONS + 12 bytes per slot
 * (128 KiB; 8 MiB for 64 slots) plus staging buffers that grow with the largest call.
 *
 * Refused with SDM_EINVAL, that slot's observations left absent and the batch's other keyframes stored: n_kp or n_depths
 * above SDM_MAX_OBSERVATIONS, a non-negative id that appears twice (the host helper would emit the cross product; the
 * fork never holds one map point at two keypoints, MapPoint.cc:103-106 and 209-216), a NaN or infinite angle.  A bad
 * argument (null pointer, negative count, slot out of range, a slot twice in one batch) refuses the whole call before
 * anything changes.  Arrays may be NULL where their count is 0.  Host-blocking (one status read-back); every caller
 * buffer is free on return. */
int sdm_upload_observations(sdm_ctx *ctx, int slot, int n_kp, const int *map_point_ids, const float *angles,
                            int n_depths, const float *depths);
/* n keyframes in one packed host-to-device copy and one kernel launch */
int sdm_upload_observations_batch(sdm_ctx *ctx, int n, const int *slots, const int *n_kp,
                                  const int *const *map_point_ids, const float *const *angles, const int *n_depths,
                                  const float *const *depths);
/* rot_deg [n_ref][n] (may be NULL), min_depth / max_depth [n_ref] (may be NULL): host arrays, written on return.
 * SDM_ESTATE for a slot without observations; SDM_EINVAL for a reference without depths when a bound is asked for
 * (the host helper's n <= 0 refusal), n outside [1, max_neighbours], a slot out of range.  One copy in, one launch,
 * one copy out, then a stream synchronise: the host needs the priors before K1 is set up. */
int sdm_search_priors(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n, const int *nbr_slots, float *rot_deg,
                      float *min_depth, float *max_depth);
/* sdm_search_priors + sdm_recon: the same maps as sdm_recon fed the host helpers' values */
int sdm_recon_observed(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n, const int *nbr_slots);

/* ---- covisible neighbours from the same observations, on the device -----------------------------
 * What SemiDenseRecon does first (PM.cc:151-160): take the first n usable keyframes of the reference's covisibility
 * order.  ref_slots[n_ref] are the references; cand_slots[n_cand] the keyframes the caller considers usable (PM.cc:156-157:
 * not bad, Mapped()).  All of them must hold observations.
 *
 * Weight w(r, c): the number of distinct map-point ids >= 0 uploaded for both slots; the angle is not looked at
 * (KeyFrame::UpdateConnections, KeyFrame.cc:302-320, counts every map point of the keyframe).  A candidate whose slot is
 * the reference's has weight 0 and is never selected (KeyFrame.cc:316).
 * Connected list of r (KeyFrame.cc:326-361): the candidates with w >= min_weight, by w descending; equal weights by
 * position in cand_slots, ascending.  If none reaches min_weight but the largest weight is >= 1, the list is the one
 * candidate with the largest weight, the earliest position among equals (KeyFrame.cc:348-352).  If every weight is 0 the
 * list is empty (KeyFrame.cc:323).  SDM_COVIS_MIN_WEIGHT is the reference's th.
 * The tie rule is a normative choice: the reference orders equal weights by KeyFrame pointer value, which no caller can
 * reproduce; list position is the deterministic stand-in.
 * Neighbours: the first n entries of the connected list.  counts[r] = min(n, its length); unused entries of nbr_slots are
 * -1, of nbr_weights 0.
 *
 * SDM_ESTATE for a reference or candidate slot without observations.  SDM_EINVAL for a null pointer, n outside
 * [1, max_neighbours], n_cand < 1, a slot out of range, a slot twice in cand_slots or twice in ref_slots, min_weight < 1.
 * A reference may also be a candidate.  A refused call changes nothing, the output arrays included.  One copy in, two
 * launches (one for sdm_covisibility), one copy out, one stream synchronise: the host needs the table before the search
 * can be set up. */
#define SDM_COVIS_MIN_WEIGHT 15                     /* KeyFrame.cc:330 */

/* weights[n_ref][n_cand] (host), row-major: shared map points of every (reference, candidate) pair */
int sdm_covisibility(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n_cand, const int *cand_slots, int *weights);

/* nbr_slots[n_ref][n] (-1 padded), nbr_weights[n_ref][n] or NULL, counts[n_ref] or NULL: host arrays */
int sdm_covisible_neighbours(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n_cand, const int *cand_slots,
                             int n, int min_weight, int *nbr_slots, int *nbr_weights, int *counts);

/* PM.cc:151-231 for a batch: choose the neighbours, derive the priors, reconstruct (sdm_covisible_neighbours, then
 * sdm_recon_observed on the references that have n neighbours).
 * done[r] = 1 if reference r had n neighbours and was reconstructed.
 * done[r] = 0 if it had fewer: PM.cc:160 skips such a keyframe.  Its slot is left exactly as it was.
 * nbr_slots_out [n_ref][n] may be NULL.  A refusal of sdm_recon_observed (a reference without an image or without point
 * depths) is returned as it is, with done and nbr_slots_out unwritten. */
int sdm_recon_covisible(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n_cand, const int *cand_slots,
                        int n, int min_weight, int *nbr_slots_out, unsigned char *done);

/* ---- InterKeyFrameDepthChecking, PM.h:91 / PM.cc:628-799 -------------------------------------- */
/* Reads the neighbours' current {rho,sigma}; writes the checked rho of each reference keyframe to
 * its "checked" plane.  commit != 0 also stores it back into the keyframe's depth map, which is
 * the reference's in-place behaviour (call with n_ref = 1, in the caller's keyframe order). */
int sdm_inter_check(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n, const int *nbr_slots,
                    int commit);

/* Precondition (the reference's gate at PM.cc:292-298: the keyframe and ALL its neighbours have
 * semidense_flag_ set): every reference and neighbour slot must hold a depth map -- produced by sdm_recon /
 * sdm_search_fuse, restored by sdm_upload_depth, received by an sdm_exchange_* call, or declared with
 * sdm_assume_pipeline_maps / sdm_mark_depth_present.  Otherwise SDM_ESTATE. */

/* ---- UpdateSemiDensePointSet, PM.h:88 / PM.cc:337-367 ----------------------------------------- */
/* source: 0 = depth map, 1 = checked plane.  Needs with_pointset. */
int sdm_pointset(sdm_ctx *ctx, int n_ref, const int *ref_slots, int source);
/* sdm_inter_check followed by sdm_pointset(source = 1) -- the pair the reference runs per ready keyframe
 * (PM.cc:300-306) -- with the back-projection done in the checking kernel when the maps came out of
 * SemiDenseRecon; identical results to the two calls. */
int sdm_inter_check_pointset(sdm_ctx *ctx, int n_ref, const int *ref_slots, int n, const int *nbr_slots,
                             int commit);

/* ---- map transfer ------------------------------------------------------------------------------ */
int sdm_upload_depth(sdm_ctx *ctx, int slot, const float *rho, const float *sigma);
int sdm_download_depth(sdm_ctx *ctx, int slot, float *rho, float *sigma); /* depth_map_/depth_sigma_ */
int sdm_download_checked(sdm_ctx *ctx, int slot, float *rho);
int sdm_download_pointset(sdm_ctx *ctx, int slot, float *xyz);            /* H x 3W */
/* ---- the filtered semi-dense point cloud ----------------------------------------------------------- */
/* The points every consumer of a finished keyframe keeps (SavePointCloudObj PM.cc:100-132, the transcript writer,
 * the adapter's hand-over): pixel (y, x) passes iff !((double)sigma > max_sigma) && (double)rho > min_rho -- a NaN
 * sigma passes, a NaN rho fails; the reference's values are max_sigma = 0.01, min_rho = 0.000001.  Extracted on the
 * device so that only the points cross the link, in the host loops' order: the slots in the order given, raster
 * order within each.  Bit-identical to the filter applied to sdm_download_depth / _checked / _pointset.
 * Any field pointer may be NULL (at least one must not be). */
typedef struct {
    float *xyz;          /* [capacity][3] world point (SemiDensePointSets_), or NULL */
    unsigned *pixel;     /* [capacity] (y << 16) | x, or NULL */
    float *rho_sigma;    /* [capacity][2] the rho that passed and its sigma, or NULL */
    uint8_t *intensity;  /* [capacity] im(y,x), or NULL */
    long long capacity;  /* points the buffers hold */
    int on_device;       /* 1: the pointers are device memory of this context's GPU */
} sdm_point_buffers;

/* Points of n slots that pass !(sigma > max_sigma) && rho > min_rho, slot order then raster order.
 * offsets[n+1] (host) receives each slot's first point; offsets[n] = total.
 * source: where rho comes from -- 1 = the checked plane (what SemiDenseReconBlock downloads into depth_map_),
 * 0 = the depth map; sigma is always the depth map's.  xyz is copied from the point-set plane as stored.
 * SDM_EINVAL: null ctx / out / offsets, no field requested, bad or repeated slot, and total > capacity (offsets
 * are filled, no point is written: size the buffers and call again).  SDM_ESTATE: a slot without a depth map,
 * source = 1 on a slot never inter-keyframe checked, xyz on a context without with_pointset.
 * With on_device = 1, SDM_EINVAL also for xyz / pixel not 4-byte and rho_sigma not 8-byte aligned.
 * Queued on the context's stream; one host wait in the middle (the total), host destinations (pageable or
 * sdm_host_alloc) are filled by one copy per field of exactly total points from an engine-owned staging buffer;
 * returns after a stream sync.  Like every compute call, it first waits for the list lengths of its slots if an
 * upload's read-back of them is still in flight (the tiles are cut on the host).  Changes no plane, flag, list or
 * counter.
 * Cost: a slot whose rho plane is zero outside its active list (maps of SemiDenseRecon) is walked through the list
 * when a zero rho fails (min_rho >= 0), any other slot pixel by pixel over W x H.  Each pass (count, write) reads per walked pixel 8 B {rho,sigma}
 * + 4 B checked rho (source 1) + 4 B list entry (list walk): 32 B per listed pixel over both passes at source 1;
 * each written point reads 12 B xyz (+ 16 B record line for intensity) and writes 12 + 4 + 8 + 1 B for the four
 * fields, which is also what crosses the link for a host destination. */
int sdm_extract_points(sdm_ctx *ctx, int n, const int *slots, int source, double max_sigma, double min_rho,
                       sdm_point_buffers *out, long long *offsets);
/* sdm_extract_points plus, per point, which neighbour keyframes confirm it: the point's visibility list (the
 * `KF_ind1, ..., KF_indN` of the transcript's `new point:` line).  Same points, order, offsets and fields as
 * sdm_extract_points for the same arguments; in addition support[p], p < total, is a 64-bit word whose bit j is set iff
 * the statement of PM.cc:677-755, run for neighbour nbr_slots[i * n_nbr + j] of the point's slot slots[i] on the state
 * at the time of the call, counts that neighbour (`nj >= 1`, PM.cc:755) -- the set behind the count
 * InterKeyFrameDepthChecking compares with lambdaN.
 *   - the point's rho in that statement is the rho of its slot's DEPTH MAP (the plane sdm_inter_check reads), whatever
 *     `source` selects for the filter; the neighbour's {rho, sigma} are its current depth map; the arithmetic is
 *     sdm_inter_check's (bit-identical decisions, its guard and exact fallback included);
 *   - the word is 0 for a pixel outside the 2-px inset (PM.cc:659-660) and for a pixel whose depth-map rho is skipped by
 *     PM.cc:662 ((double)rho < 1e-6); bits >= n_nbr are 0; lambdaN plays no part.
 * Consequences: after sdm_inter_check(commit = 0) on the same neighbour table the words reproduce the check's own
 * decisions -- for every inset pixel not skipped by PM.cc:662, popcount < lambdaN => checked rho == 0, and
 * checked rho != 0 => popcount >= lambdaN.  After commit = 1 the words are evaluated at the committed rho.
 * support[out->capacity] follows out->on_device (8-byte aligned there) and is a separate argument: sdm_point_buffers
 * keeps its layout.  All four field pointers may be NULL.
 * Errors: those of sdm_extract_points (total > capacity: offsets filled, nothing written) and of sdm_inter_check's
 * neighbour table: SDM_EINVAL for NULL support / nbr_slots, n_nbr < 1 or > max_neighbours, a neighbour slot out of
 * range (a repeated neighbour is accepted, as there); SDM_ESTATE for a slot without an uploaded keyframe or a neighbour
 * without a depth map.
 * Changes no plane, flag or list.  Staging the pair tables counts in sdm_stats::table_stagings as for any compute call,
 * and the staged set is shared with an sdm_inter_check over the same lists.
 * Cost on top of sdm_extract_points: one lane per point runs K4's per-neighbour statement n_nbr times (a subset of
 * sdm_inter_check's work on a subset of its pixels) and 8 B per point are written (and cross the link for a host
 * destination); 4 B per point of staged pixel codes when `pixel` is NULL. */
int sdm_extract_points_support(sdm_ctx *ctx, int n, const int *slots, int n_nbr, const int *nbr_slots /*[n][n_nbr]*/,
                               int source, double max_sigma, double min_rho, sdm_point_buffers *out,
                               unsigned long long *support /*[out->capacity]*/, long long *offsets);
/* sdm_extract_points merged to one point per voxel ACROSS the slots of the call: every keyframe re-observes the surface
 * its neighbours have mapped, so the plain cloud holds a surface patch once per keyframe that sees it.  Nothing in the
 * reference merges the cloud; the semantics below are this library's and are a pure function of the arguments and the
 * planes (tests/voxel_np.py restates them in NumPy).
 *   - Plain cloud: g = 0 .. T-1 are the points sdm_extract_points returns for the same (slots, source, max_sigma,
 *     min_rho), in its order; xyz is the point-set plane as stored, sigma the depth map's.
 *   - Cell: inv = 1.0f / voxel_size (one float division, on the host); c_k = floorf(xyz_k * inv), one float multiply
 *     per coordinate, never fused.  A point is MERGEABLE iff -2^20 <= c_k < 2^20 for all three k (a NaN or +-Inf
 *     coordinate fails); its voxel is the integer triple.  An unmergeable point is always kept, with multiplicity 1,
 *     and is its own representative.
 *   - Winner: among the mergeable points of one voxel the kept one minimises (key(sigma), g) lexicographically, where
 *     with u = the bits of sigma, key(sigma) = u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000) -- the order-preserving map
 *     of the float order onto unsigned integers, total on bit patterns: -0 < +0, and a NaN has a defined place (above
 *     +Inf with the sign bit clear, below -Inf with it set).  So: the smallest sigma wins; ties go to the slot listed
 *     earlier in the call, then to raster order.
 *   - Output: the kept points in plain order.  The fields of `out` carry the kept point's own values (nothing is
 *     averaged); offsets[i], i < n, is the first kept point of slot i, offsets[n] the kept total M.
 *     multiplicity[k] = plain points in kept point k's voxel; source_index[k] = its g (strictly increasing);
 *     representative[g] = the k of the point kept for plain point g, so representative[source_index[k]] == k and a
 *     visibility word of sdm_extract_points_support (same arguments, index g) can be attached to point k.
 *     vox->plain_total = T whenever the call gets as far as counting.
 * `vox` may be NULL, and so may each pointer in it; its pointers follow out->on_device and must be 4-byte aligned there
 * (multiplicity and source_index hold out->capacity entries, representative rep_capacity).  sdm_point_buffers keeps its
 * layout; all four field pointers may be NULL if `vox` names a destination.
 * Errors: those of sdm_extract_points; SDM_EINVAL also for a voxel_size that is not finite and > 0 or whose inv is not
 * finite (a denormal size), no destination at all, a misaligned device pointer, T >= 2^32 - 1 (in this implementation:
 * T > 2^30, whose table would pass 2^31 slots), and M > out->capacity or (representative != NULL and
 * T > rep_capacity) -- in these two cases offsets and plain_total are filled and nothing is written.  SDM_ESTATE on a
 * context without with_pointset even when out->xyz is NULL: the merge reads the plane.  SDM_EHIP "voxel table overflow"
 * cannot happen (the probe of a table at most half full always ends) and is reported rather than looped on.
 * Changes no plane, flag, list or counter, exactly like sdm_extract_points.  Bitwise reproducible from run to run.
 * Cost: sdm_extract_points' passes with xyz and rho_sigma (plus the requested pixel / intensity) written to an
 * engine-owned staging, 20 B (+ 4 + 1 B) per plain point; then per plain point one probe of a hash table (three integer
 * atomics: a 64-bit compare-and-swap, a 64-bit min, a 32-bit add) and 4 B of table position, two more passes over those
 * 4 B and the 8 B table value, and per KEPT point a gather of the requested fields (12 + 4 + 8 + 1 B read and written)
 * + 4 B multiplicity + 4 B source_index; 4 B per plain point for representative.  Only the kept points (and the
 * representative array) cross the link for a host destination, one copy per output of exactly M (T) elements.
 * Scratch in the context, grown on demand and freed by sdm_destroy: the table has the power of two >= 2 T (at least
 * 1024) slots of 24 B -- at most 96 B per plain point -- cleared per call on the stream, plus 4 B per plain point.
 * Three host waits: the plain total T, the kept total M, the end. */
typedef struct {
    unsigned *multiplicity;    /* [out->capacity] plain points that fell into the kept point's voxel (1 if unmergeable), or NULL */
    unsigned *source_index;    /* [out->capacity] index of the kept point in the plain extraction, or NULL */
    unsigned *representative;  /* [rep_capacity] per PLAIN point: index in the merged cloud of the point kept for it, or NULL */
    long long rep_capacity;
    long long plain_total;     /* out: number of points sdm_extract_points returns for the same arguments */
} sdm_voxel_buffers;
int sdm_extract_points_voxel(sdm_ctx *ctx, int n, const int *slots, int source, double max_sigma, double min_rho,
                             float voxel_size, sdm_point_buffers *out, sdm_voxel_buffers *vox /* or NULL */,
                             long long *offsets);
/* sdm_extract_points_voxel plus, per KEPT point, the cameras that saw the surface element it stands for: the
 * `new point: [x; y; z], KF_ind1, ..., KF_indN` of the transcript for the merged cloud.  Bit j of a support word names a
 * different keyframe for every slot, so the words of a voxel's points cannot be OR-ed; this call resolves them to slot
 * ids on the device and returns one list per kept point (tests/voxcam_np.py restates it in NumPy).
 *   - Unchanged outputs: the points, their order, offsets, the fields of `out` and the outputs of `vox` are exactly those
 *     of sdm_extract_points_voxel for the same (slots, source, max_sigma, min_rho, voxel_size).
 *   - Support words: with support[g] the word sdm_extract_points_support returns for the same (slots, n_nbr, nbr_slots,
 *     source, max_sigma, min_rho) at plain index g, and i(g) the position in `slots` of the slot of g,
 *         C(g) = { slots[i(g)] } U { nbr_slots[i(g)][j] : bit j of support[g] }.
 *     The observing keyframe is always a member, also when the word is 0 (outside the inset, skipped by PM.cc:662) and
 *     for an unmergeable point.
 *   - Merged list: V(k) = U { C(g) : representative[g] == k }.  The list of kept point k is V(k) as slot ids in strictly
 *     ascending order, without duplicates: cam_slots[cam_offsets[k] .. cam_offsets[k + 1]).  A repeated neighbour and a
 *     neighbour equal to the point's own slot fall out of the union; any neighbour table sdm_extract_points_support
 *     accepts is accepted here.
 *   - Offsets: cam_offsets[0] = 0 and cam_offsets[M] = cam_total = E, the sum of the list lengths.
 *   - Arithmetic: integer only; a pure function of the arguments and the planes, bitwise reproducible from run to run.
 *     Changes no plane, flag, list or counter, except sdm_stats::table_stagings as sdm_extract_points_support does (the
 *     staged set is shared with an sdm_inter_check over the same lists).
 * `cams` must not be NULL and at least one of its two pointers must not be.  With cam_slots == NULL the call returns the
 * offsets (the list lengths) only and cam_capacity is ignored.  The pointers follow out->on_device: cam_offsets 8-byte,
 * cam_slots 4-byte aligned there; cam_offsets holds out->capacity + 1 entries.  `out` and `vox` may name no destination
 * at all.
 * Errors: the union of sdm_extract_points_voxel's and sdm_extract_points_support's (NULL cams / nbr_slots, no camera
 * pointer, a negative cam_capacity, a misaligned device pointer, n_nbr < 1 or > max_neighbours, a neighbour slot out of
 * range: SDM_EINVAL; a neighbour without a depth map: SDM_ESTATE), all checked on the host before anything is queued.
 *   - M > out->capacity and (representative != NULL and T > rep_capacity) come first and keep their contract: offsets
 *     and plain_total filled, nothing written, cam_total = 0.
 *   - E > cam_capacity with cam_slots != NULL: SDM_EINVAL with offsets, plain_total and cam_total filled; neither camera
 *     array is written, the content of the other destinations is unspecified.  Size cam_slots and call again.
 *   - SDM_EINVAL also when min(M, 2^22) x (distinct slots of the call) >= 2^32: the list pass scans 32-bit sums.
 * Cost on top of sdm_extract_points_voxel: sdm_extract_points_support's pass over the T plain points (4 B of staged pixel
 * codes and 8 B of support word per plain point) and, when the caller takes no `representative`, its 4 B per plain
 * point in engine scratch; then per plain point 12 B read (word, rank) and at most Wd = ceil(Cn / 64) 64-bit atomic ORs,
 * Cn the distinct slots among slots and nbr_slots -- the lanes of a wave that share a kept point combine first, so a
 * run of equal ranks issues one atomic per word; per kept point Wd x 8 B of bitset (cleared per call on the stream, read
 * twice), 8 B of offset and 4 B per list entry written.  Only cam_offsets (8 (M + 1) B) and cam_slots (4 E B) cross the
 * link for a host destination.  Scratch lives in the context, grows on demand and is freed by sdm_destroy.
 * Four host waits: the plain total T, the kept total M, the lists' total E, the end. */
typedef struct {
    long long *cam_offsets;   /* [out->capacity + 1]: list of kept point k = cam_slots[cam_offsets[k] .. cam_offsets[k+1]), or NULL */
    int *cam_slots;           /* [cam_capacity] slot ids, or NULL */
    long long cam_capacity;
    long long cam_total;      /* out: sum of the list lengths E */
} sdm_voxel_cameras;
int sdm_extract_points_voxel_cameras(sdm_ctx *ctx, int n, const int *slots, int n_nbr, const int *nbr_slots /*[n][n_nbr]*/,
                                     int source, double max_sigma, double min_rho, float voxel_size,
                                     sdm_point_buffers *out, sdm_voxel_buffers *vox /* or NULL */,
                                     sdm_voxel_cameras *cams, long long *offsets);
/* sdm_extract_points_voxel_cameras plus free-space evidence: per KEPT point k, crossings[k] = the number of (camera,
 * kept point) rays of the call that pass through k's voxel on their way to another point -- the voxel-level form of the
 * question the reference's carving asks of a (camera, point) ray.  Nothing in the reference counts it; the semantics
 * below are this library's (tests/carve_np.py restates them in NumPy).  Every other output is, byte for byte, what
 * sdm_extract_points_voxel_cameras returns for the same arguments.
 * All arithmetic is IEEE binary32 without fused multiply-add and with correctly rounded division.
 *   - Rays: one per entry of the camera lists, e in [0, E): kept point k(e) (cam_offsets[k] <= e < cam_offsets[k + 1]) and
 *     camera slot s(e) = cam_slots[e].  The ray ends in P, the kept point's returned xyz.
 *   - Origin: O = the camera centre of slot s from its CURRENT pose (sdm_set_pose counts), formed as the point-set pass
 *     forms it: Rwc[i][j] = Tcw[j*4+i], Ow_i = (Rwc[i][0]*t0 + Rwc[i][1]*t1) + Rwc[i][2]*t2 with t = (Tcw[3], Tcw[7],
 *     Tcw[11]), O = -Ow; computed on the host per distinct camera of the call.
 *   - Cells: inv = 1.0f / voxel_size as for sdm_extract_points_voxel; cO_a = floorf(O_a * inv), cP_a = floorf(P_a * inv).
 *     A ray is SKIPPED -- it touches nothing and adds 1 to rays_skipped -- if any of the six cells is not in
 *     [-2^20, 2^20) (every compare is false for a NaN: an unmergeable end point or a non-finite pose skips), or if
 *     N = sum_a |cP_a - cO_a| > max_steps.
 *   - Walk: integer-driven, exactly N steps, ending exactly in cP.  step_a = sign(cP_a - cO_a), r_a = |cP_a - cO_a|,
 *     d_a = P_a - O_a.  For the axes with r_a > 0: bnd_a = (float)(cO_a + (step_a > 0 ? 1 : 0)) * voxel_size,
 *     tMax_a = (bnd_a - O_a) / d_a, tDel_a = voxel_size / fabsf(d_a).  cur = cO; for s = 0 .. N-1: cur is the ray's cell
 *     of index s; the axis a with r_a > 0 and the smallest tMax_a is chosen -- x, y, z are scanned in turn and an axis
 *     replaces the choice only if its tMax is strictly smaller, so ties and NaNs go to the earlier axis -- and then
 *     cur_a += step_a, r_a -= 1, tMax_a = tMax_a + tDel_a.  Axes with r_a = 0 are never read.
 *   - Counting: the cells of index s <= N - 1 - end_margin are counted: the camera's own cell s = 0 is, the end cell
 *     s = N never.  For each counted cell that is the voxel of a mergeable kept point j, crossings[j] += 1.
 *     cells_visited adds max(0, N - end_margin) per walked ray.  An unmergeable kept point has crossings 0.
 *   - crossings and the totals are integer sums: a pure function of the arguments, the planes and the poses, bitwise the
 *     same from run to run.  The call changes no plane, flag, list or counter beyond what
 *     sdm_extract_points_voxel_cameras touches.
 * `cams` follows sdm_extract_points_voxel_cameras' rules except that both of its pointers may be NULL: the lists are then
 * formed in engine scratch and cam_capacity is ignored (cam_total is still returned).  `out` and `vox` may name no
 * destination.  crossings follows out->on_device (4-byte aligned there) and holds out->capacity entries.
 * Errors: every refusal of the composed calls, with its contract and in its order (offsets, plain_total and cam_total
 * filled as there); SDM_EINVAL, checked on the host before anything is queued, also for fs == NULL, crossings == NULL,
 * end_margin < 0, max_steps outside 1 .. SDM_FREESPACE_MAX_STEPS and a misaligned device pointer; SDM_EINVAL for
 * E >= 2^32.  On any refusal crossings is not written and rays_total, rays_skipped and cells_visited are 0.
 * Cost on top of sdm_extract_points_voxel_cameras: one lane per ray; per ray a binary search in cam_offsets (at most 33
 * 8-byte reads) and in the camera table, 12 + 16 B of end point and centre, six float divisions; per counted cell one
 * read-only probe of the voxel table (8 B keys until the equal key or an empty slot; at load <= 0.5 a probe and a half on
 * average) and, on a hit, 4 B of rank and one 32-bit atomic add.  The probes of one ray depend on nothing but the walk, so
 * the pass is bound by their latency, not by bandwidth.  4 B per kept point are cleared and written (and cross the link
 * for a host destination); two 64-bit atomics per wave carry the totals.  Engine scratch, grown on demand and freed by
 * sdm_destroy: 16 B per distinct camera, and 12 B per kept point / 8 B per kept point / 4 B per ray for the xyz and the
 * lists the caller names no device destination for.  No host wait beyond sdm_extract_points_voxel_cameras' four: the
 * totals come back with the last one. */
#define SDM_FREESPACE_MAX_STEPS 65536
typedef struct {
    unsigned *crossings;      /* [out->capacity] rays that traverse kept point k's voxel; follows out->on_device, 4-byte aligned; must not be NULL */
    int end_margin;           /* in: >= 0; the last end_margin cells before the ray's end cell are not counted */
    int max_steps;            /* in: 1 .. SDM_FREESPACE_MAX_STEPS (65536); a longer ray is skipped, not truncated */
    long long rays_total;     /* out: E = cam_total */
    long long rays_skipped;   /* out: rays not walked (rules above) */
    long long cells_visited;  /* out: counted (ray, cell) pairs over all walked rays */
} sdm_voxel_freespace;
int sdm_extract_points_voxel_freespace(sdm_ctx *ctx, int n, const int *slots, int n_nbr, const int *nbr_slots /*[n][n_nbr]*/,
                                       int source, double max_sigma, double min_rho, float voxel_size,
                                       sdm_point_buffers *out, sdm_voxel_buffers *vox /* or NULL */,
                                       sdm_voxel_cameras *cams, sdm_voxel_freespace *fs, long long *offsets);
/* ---- the persistent voxel map ------------------------------------------------------------------------ */
/* sdm_extract_points_voxel merges within one call.  The voxel map keeps the merge in the context ACROSS calls: each
 * sdm_vmap_integrate merges the plain cloud of its slots into the entries left by the calls before it and reports exactly
 * what changed, so an online consumer (one keyframe or one block per call) appends the created entries and rewrites the
 * updated ones without re-reading the cloud.  Nothing in the reference does this; the semantics below are this library's
 * and make the map a pure function of the sequence of calls (tests/vmap_np.py restates them in NumPy).
 * One map per context, optional.  voxel_size, inv = 1.0f / voxel_size, the cell floorf(xyz_k * inv), mergeability (all
 * three cells in [-2^20, 2^20), every compare false for a NaN) and key(sigma) are exactly sdm_extract_points_voxel's.
 *   - State: entries id = 0 .. M-1, one per distinct voxel ever seen.  An entry carries the record of its winning point
 *     -- xyz, pixel, rho_sigma, intensity as sdm_extract_points returns them, and tag (int) -- plus multiplicity (u32)
 *     and epoch (u32, the number of the call whose point is the winner).  Counters: points, dropped, calls, rehashes.
 *   - Integrating: call number c counts the successful sdm_vmap_integrate calls since open or clear, from 1.  Its plain
 *     cloud g = 0 .. T-1 is what sdm_extract_points returns for (n, slots, source, max_sigma, min_rho) on the state at
 *     the time of the call, in its order; xyz is the point-set plane as stored.  A point's tag is tags[i] for its slot
 *     slots[i], or the slot number when tags == NULL (slots are recycled in an online run: pass the keyframe ids).
 *     The result is defined as if the points were processed one by one in increasing g:
 *       * an unmergeable point adds 1 to `dropped` and is not stored (the one deliberate difference from the per-call
 *         merge, which keeps such points: a voxel map has no voxel for them);
 *       * a point whose voxel has no entry creates entry id = M: its record is the point, multiplicity = 1, epoch = c;
 *         then M += 1;
 *       * otherwise multiplicity += 1, saturating at 2^32 - 1, and if key(sigma_g) < the key of the entry's stored
 *         sigma, STRICTLY, the record becomes the point and epoch = c.
 *     `points` adds the mergeable points (a 64-bit sum).
 *     So an entry's winner minimises (key(sigma), G) over the concatenation G of all integrated plain clouds in call
 *     order: the smallest sigma wins, ties go to the earlier call, then the earlier slot, then raster order.  Ids are the
 *     order of each voxel's FIRST point in G: append-only, they never change.
 *   - Delta of call c: first_created = M before the call; created = entries appended, with ids first_created ..
 *     first_created + created - 1; updated = entries with id < first_created whose epoch became c; updated_ids lists
 *     those ids in ascending order of the plain index g of the entry's final winner in this call; plain_total = T;
 *     dropped = this call's dropped points.
 *   - Invariants: integrating slots s0 .. sk in one call, in k+1 calls of one slot, or in any split into consecutive
 *     groups leaves a byte-identical map except `epoch` and `calls`.  One call into an empty map gives, matched by
 *     (tag, pixel), exactly the mergeable kept points of sdm_extract_points_voxel for the same arguments, with the same
 *     field bits and multiplicities, and `dropped` = its unmergeable kept points.  Integrating the same slots again
 *     with unchanged planes gives created = 0, updated = 0 and doubles every multiplicity.
 * Everything is integer or copied bits: every returned array is bitwise the same from run to run.
 * sdm_vmap_open: reserve_voxels sizes the table (the power of two >= 2 x reserve_voxels, at least 1024 slots) and the
 * records; 0 = the minimum.  sdm_vmap_clear: an empty map as after open (all counters 0), the capacity kept.
 * sdm_vmap_close frees the map; sdm_destroy does too.
 * sdm_vmap_fetch returns entries first .. first + count - 1 when ids == NULL, else entries ids[0 .. count) (first must
 * be 0 then).  ids and the pointers of `extra` follow out->on_device and are 4-byte aligned there (rho_sigma: 8).  Any
 * pointer of `out` and `extra` may be NULL, and so may `extra`; at least one destination must be named.
 * sdm_point_buffers keeps its layout.
 * Errors, all raised before the map changes (a refused call leaves sdm_vmap_get_info and a full fetch as they were):
 *   SDM_ESTATE: no open map; open on an open map; a context without with_pointset; the slot states sdm_extract_points
 *     refuses.
 *   SDM_EINVAL: sdm_extract_points' argument errors; a voxel_size sdm_extract_points_voxel refuses; negative
 *     reserve_voxels (or more than 2^30); a misaligned device pointer; updated_ids != NULL with updated_capacity <
 *     min(M, T), the a-priori bound on `updated` (plain_total and first_created are filled); M + T > 2^30 (the table would
 *     pass 2^31 slots); fetch: count < 0, count > out->capacity, a range beyond M, an id >= M (device ids: a kernel flag
 *     read at the final wait; the destinations are then unspecified), first != 0 with ids, no destination.
 *   SDM_EHIP: an allocation failure while growing -- growth is done before anything is inserted.
 * Changes no plane, flag, list or counter of the engine, and uses scratch of its own: interleaved
 * sdm_extract_points_voxel* calls are undisturbed.
 * Cost per sdm_vmap_integrate, outside a growth proportional to T and not to M or the table: sdm_extract_points' passes
 * with all four fields staged (25 B per plain point); per plain point one probe of the table with four integer atomics
 * (a 64-bit compare-and-swap, a 64-bit min, a 32-bit min, a 32-bit add) and 4 B of table position; three more passes over
 * those 4 B and the table fields; per created or updated entry a 37 B record.  Growth: when 2 (M + T) exceeds the table's
 * slots a table of the next sufficient power of two is made and every old slot re-inserted (`rehashes` counts these);
 * the records grow geometrically by device copies.  Memory: 28 B per table slot, 37 B per record.  Three host waits: T,
 * the counts, the end.  sdm_vmap_fetch: one copy per field of exactly count elements (range form), after one gather
 * launch (ids form).
 * Limits: a keyframe's contribution cannot be removed by these calls (sdm_vmap_retire, below, removes it); stored xyz go stale after sdm_set_pose (remedy: sdm_vmap_clear and
 * integrate the resident slots again); free-space evidence is kept per entry by sdm_vmap_carve and the camera
 * lists by sdm_vmap_observe (both below); one rank only per map: the maps of several ranks, a saved map or a map of
 * another voxel_size come in through sdm_vmap_import (below).  Under adjusted poses sdm_vmap_repose (below) re-places
 * the stored points without the slots. */
typedef struct {
    long long voxels;       /* M */
    long long points;       /* mergeable points integrated */
    long long dropped;      /* unmergeable points met */
    long long calls;        /* successful sdm_vmap_integrate and sdm_vmap_import calls since open / clear */
    long long table_slots;
    long long rehashes;     /* table growths since open / clear */
    float voxel_size;
} sdm_vmap_info;
typedef struct {
    unsigned *updated_ids;        /* in: [updated_capacity] or NULL */
    long long updated_capacity;   /* in */
    int on_device;                /* in: 1: updated_ids is device memory of this context's GPU (4-byte aligned) */
    long long plain_total;        /* out: T */
    long long dropped;            /* out */
    long long first_created;      /* out: M before the call */
    long long created;            /* out */
    long long updated;            /* out */
} sdm_vmap_delta;
typedef struct {
    int *tag;                 /* [out->capacity] or NULL */
    unsigned *multiplicity;   /* [out->capacity] or NULL */
    unsigned *epoch;          /* [out->capacity] or NULL */
} sdm_vmap_fields;
int sdm_vmap_open(sdm_ctx *ctx, float voxel_size, long long reserve_voxels);
int sdm_vmap_clear(sdm_ctx *ctx);
int sdm_vmap_close(sdm_ctx *ctx);
int sdm_vmap_get_info(sdm_ctx *ctx, sdm_vmap_info *info);
int sdm_vmap_integrate(sdm_ctx *ctx, int n, const int *slots, const int *tags /*[n] or NULL*/, int source,
                       double max_sigma, double min_rho, sdm_vmap_delta *delta /* or NULL */);
int sdm_vmap_fetch(sdm_ctx *ctx, const unsigned *ids /*[count] or NULL*/, long long first, long long count,
                   sdm_point_buffers *out, sdm_vmap_fields *extra /* or NULL */);
/* Free-space evidence on the persistent map: the (camera, point) rays of a call are walked through the map's table on
 * the device and counted per ENTRY, so an online caller integrates a finished block, carves it, and fetches the counters by
 * id like every other field.  Nothing in the reference counts this; the semantics below are this library's
 * (tests/vmap_carve_np.py restates them in NumPy).
 *   - State: every entry carries two 64-bit counters, crossings and ends.  Both are 0 when the entry is created;
 *     sdm_vmap_clear puts both back to 0.  (64 bits: the voxel at a camera centre collects every ray of that camera, and
 *     no realistic sequence wraps them.)
 *   - Plain cloud: sdm_vmap_carve reads the plain cloud g = 0 .. T-1 of (n, slots, source, max_sigma, min_rho) exactly as
 *     sdm_vmap_integrate does.
 *   - Cameras of a point: with n_nbr >= 1 it also reads the support words of sdm_extract_points_support for the same
 *     arguments; C(g) = {slots[i(g)]} U {nbr_slots[i(g)][j] : bit j of support[g]}, i(g) the index of the point's slot.
 *     C(g) is a SET: a repeated neighbour and a neighbour equal to the point's own slot fall out.  n_nbr == 0 with
 *     nbr_slots == NULL is allowed: C(g) is then the observing slot alone and no support pass runs.
 *   - Rays: one per (g, s in C(g)), from O, the camera centre of slot s from its CURRENT pose -- formed on the host
 *     exactly as sdm_extract_points_voxel_freespace forms it, once per distinct camera of the call -- to P, the plain
 *     point's own staged xyz (not the entry's record).  The skip rule, the cells, the integer-driven walk of exactly N
 *     steps, the tie rule and the counted cells s <= N - 1 - end_margin are sdm_extract_points_voxel_freespace's, word for
 *     word, with the map's voxel_size and inv.  A non-finite or out-of-range point or centre skips its ray.
 *   - Counting: for every counted cell whose key has an entry, crossings[id] += 1.  For every walked (not skipped) ray
 *     whose end cell cP has an entry, ends[id] += 1, whatever end_margin.
 *   - The map is read, not changed: nothing is inserted; no id, record, multiplicity, epoch or counter of
 *     sdm_vmap_get_info changes.  Evidence is therefore relative to the entries present at the call: integrate a block,
 *     then carve it.
 *   - Everything is an integer sum: the counters and totals are bitwise the same from run to run, whatever the table
 *     layout.  For a fixed map carving is additive over any split or order of the slots into calls.  The counters survive
 *     table rehashes and record growth; entries created later start at 0.
 * sdm_vmap_fetch_evidence follows the range and ids forms of sdm_vmap_fetch (ids follow ev->on_device, 4-byte aligned
 * there; crossings and ends 8-byte aligned); it returns zeros if no carve has run; at least one destination must be named.
 * Errors, all raised before any counter changes: SDM_ESTATE for no open map and the slot and neighbour states
 * sdm_extract_points and sdm_extract_points_support refuse; SDM_EINVAL for their argument errors, cv == NULL,
 * end_margin < 0, max_steps outside 1 .. SDM_FREESPACE_MAX_STEPS, n_nbr < 0, n_nbr > max_neighbours, n_nbr == 0 with a
 * table and n_nbr >= 1 without one, and the fetch errors exactly as sdm_vmap_fetch (range beyond M, count > capacity, an
 * id >= M, first != 0 with ids, a misaligned device pointer, no destination); SDM_EHIP for an allocation failure --
 * everything is allocated before anything is counted.  On a refusal the outs of cv are 0, except plain_total once known.
 * Cost: sdm_extract_points' passes (20 B per plain point staged) and, with neighbours, sdm_extract_points_support's pass;
 * one lane per candidate (g, d), d = 0 .. D, D = the most distinct neighbours of one slot; per live ray six float
 * divisions and per counted cell one read-only probe of the table (8 B keys; on a hit 4 B of id and one 64-bit atomic
 * add), plus one probe for the end cell.  The probes of a ray depend on the walk alone: the pass is bound by their latency.
 * Memory: 16 B per record of capacity, allocated at the first carve.  Two host waits: T, the end (with the totals).
 * Limits: evidence is relative to the entries present at each carve, so -- unlike the map itself -- it is NOT invariant
 * under re-splitting integrates and carves against each other; carving the same slots twice counts twice; the counters go
 * stale with sdm_set_pose, as the stored xyz do; a keyframe's contribution cannot be removed from the counters
 * (sdm_vmap_retire, below, removes its entries and pairs, and its carry = 1 keeps the rays it added); one rank only: the
 * counters do not travel with sdm_vmap_import (below) -- carve on the merged map.  sdm_vmap_repose (below) carries or
 * restarts the counters when the poses move, and sdm_vmap_recarve (further below) makes them again from the observation
 * log when the slots that made them are gone. */
typedef struct {
    int end_margin;            /* in: >= 0 */
    int max_steps;             /* in: 1 .. SDM_FREESPACE_MAX_STEPS */
    long long plain_total;     /* out: T */
    long long rays_total;      /* out */
    long long rays_skipped;    /* out */
    long long cells_visited;   /* out: counted (ray, cell) pairs */
    long long cells_hit;       /* out: of those, cells that hold an entry = sum of the crossings added */
    long long ends_hit;        /* out: walked rays whose end cell holds an entry = sum of the ends added */
} sdm_vmap_carve_args;
typedef struct {
    unsigned long long *crossings;  /* [capacity] or NULL */
    unsigned long long *ends;       /* [capacity] or NULL */
    long long capacity;
    int on_device;                  /* pointers (and ids) are device memory, 8-byte aligned (ids: 4) */
} sdm_vmap_evidence;
int sdm_vmap_carve(sdm_ctx *ctx, int n, const int *slots, int n_nbr, const int *nbr_slots /*[n][n_nbr] or NULL*/,
                   int source, double max_sigma, double min_rho, sdm_vmap_carve_args *cv);
int sdm_vmap_fetch_evidence(sdm_ctx *ctx, const unsigned *ids /*[count] or NULL*/, long long first, long long count,
                            sdm_vmap_evidence *ev);
/* Camera lists on the persistent map, kept as an append-only observation log: every entry accumulates, across calls, the
 * set of keyframe TAGS that saw any point of its voxel, and every sdm_vmap_observe reports exactly which (entry, tag)
 * pairs are new.  An online caller integrates a finished block, observes it, and fetches the created range of the log: a
 * pair on an entry the same block created belongs to that entry's `new point: [x; y; z], KF_ind1, ..., KF_indN`, a pair on
 * an older entry is an `observation: camIndex, pointIndex`.  Nothing in the reference does this; the semantics below are
 * this library's (tests/vmap_obs_np.py restates them in NumPy).  Requires an open map; voxel_size, inv, the cell
 * floorf(xyz_k * inv) and mergeability are sdm_vmap_integrate's.
 *   - State: observations k = 0 .. E-1, each a pair (entry id, tag); no pair is stored twice.  E = 0 after sdm_vmap_open
 *     and sdm_vmap_clear; sdm_vmap_close and sdm_destroy free everything.  Log indices never change.
 *   - Plain cloud: sdm_vmap_observe reads the plain cloud g = 0 .. T-1 of (n, slots, source, max_sigma, min_rho) exactly as
 *     sdm_vmap_integrate and sdm_vmap_carve do and, with n_nbr >= 1, the support words of sdm_extract_points_support for
 *     the same arguments.  n_nbr == 0 with nbr_slots == NULL and nbr_tags == NULL is allowed, as in sdm_vmap_carve: the
 *     point's own camera is then its only one and no support pass runs.
 *   - Tags: the tag of slot slots[i] is tags[i], or the slot number when tags == NULL; the tag of column j of row i is
 *     nbr_tags[i*n_nbr + j], or nbr_slots[i*n_nbr + j] when nbr_tags == NULL.  Every tag must lie in [0, 2^31).  Tags are
 *     the persistent camera identity (slots are recycled in an online run): pass the keyframe ids, the same ones given
 *     to sdm_vmap_integrate.
 *   - Cameras of a point: C(g) = {tag(slots[i(g)])} U {tag of column j : bit j of support[g]}, i(g) the index of the
 *     point's slot.  C(g) is a SET of tags: columns with equal tags collapse, and a column whose tag equals the point's
 *     own tag falls out.
 *   - Entry of a point: id(g) = the entry of the voxel of the point's staged xyz, if the point is mergeable and the map
 *     holds that voxel; otherwise the point is UNMAPPED: it adds 1 to `unmapped` and contributes nothing.  The map is
 *     read, not changed: no id, record, multiplicity, epoch, evidence counter or field of sdm_vmap_get_info moves.  The
 *     recipe is: integrate a block, then observe it (then carve it, if evidence is wanted).
 *   - Result: defined as if the mapped points were processed in increasing g, and within a point its tags in ascending
 *     order: a pair (id(g), t) not yet stored is appended with index E, then E += 1.  `candidates` adds |C(g)| per mapped
 *     point.
 *   - Delta (sdm_vmap_observe_delta, all outs): plain_total = T, unmapped, candidates, first_created = E before the call,
 *     created; the new observations are log entries first_created .. first_created + created - 1.
 *   - Invariants: on a fixed map, observing slots s0 .. sk in one call, in k+1 calls of one slot, or in any split into
 *     consecutive groups leaves a byte-identical log.  Observing the same slots again with unchanged planes creates
 *     nothing.  After one sdm_vmap_integrate into an empty map and one sdm_vmap_observe of the same arguments with
 *     tags == nbr_tags == NULL, the list of every entry equals the cam_slots list sdm_extract_points_voxel_cameras
 *     returns for the kept point with the same (tag, pixel), and `unmapped` equals its unmergeable plain points.  On a
 *     fixed map the per-entry lists, though not the log order, are independent of the order of the calls.
 * Everything is integer: every returned array is bitwise the same from run to run.
 * sdm_vmap_fetch_observations returns log entries first .. first + count - 1 into out->entry (u32) and / or out->tag (int):
 * one plain copy per field of exactly count elements.  The pointers follow out->on_device, 4-byte aligned there.
 * sdm_vmap_fetch_cameras returns, for entries first .. first + count - 1 (ids == NULL) or ids[0 .. count) (first must be
 * 0; ids may repeat; ids follow cams->on_device, 4-byte aligned there), the tags of requested entry j in strictly
 * ascending order: cam_tags[cam_offsets[j] .. cam_offsets[j + 1]), cam_offsets[0] = 0, cam_offsets[count] = cam_total.
 * An entry never observed has an empty list.  The rules are sdm_voxel_cameras': at least one of the two pointers;
 * cam_tags == NULL gives the offsets only and cam_capacity is ignored; cam_total > cam_capacity with cam_tags != NULL is
 * SDM_EINVAL with cam_total filled and neither array written; cam_offsets holds capacity + 1 entries and is 8-byte,
 * cam_tags 4-byte aligned on the device.  Reading changes nothing, so the caller sizes cam_tags and calls again.
 * sdm_vmap_get_obs_info: observations = E, calls = successful sdm_vmap_observe calls since open / clear, table_slots and
 * rehashes of the observation set (0 slots before the first observe with a plain point).
 * Errors, all raised before any state changes (a refused call leaves the log, both infos and full fetches as they were):
 *   SDM_ESTATE: no open map; the slot and neighbour states sdm_extract_points / sdm_extract_points_support refuse.
 *   SDM_EINVAL: their argument errors; ob == NULL; a tag outside [0, 2^31); n_nbr < 0 or > max_neighbours; n_nbr == 0 with
 *     a table; n_nbr >= 1 without nbr_slots; nbr_tags without nbr_slots; E + B > 2^30, B = sum_i T_i x L_i the a-priori
 *     bound on new pairs (T_i the plain points of slot i, L_i the distinct tags of row i including its own): the set would
 *     pass 2^31 slots; T x Lmax > 2^40, Lmax the largest L_i: the candidate index space the scans address; the fetch
 *     errors exactly as sdm_vmap_fetch's (count < 0, count > capacity, a range beyond E or M, an id >= M, first != 0 with
 *     ids, a misaligned device pointer, no destination); sdm_vmap_fetch_cameras also when min(count, 2048) x (distinct
 *     tags observed since open / clear) >= 2^32: the list pass scans 32-bit sums.
 *   SDM_EHIP: an allocation failure while growing -- everything is allocated before anything is inserted.
 * On a refusal the outs of ob are 0, except plain_total once known.
 * Changes no plane, flag, list or counter of the engine except sdm_stats::table_stagings as sdm_extract_points_support
 * does, and uses scratch of its own: interleaved sdm_extract_points_voxel*, sdm_vmap_integrate and sdm_vmap_carve calls
 * are undisturbed.
 * Cost per sdm_vmap_observe: sdm_extract_points' passes (20 B per plain point staged) and, with neighbours,
 * sdm_extract_points_support's pass: proportional to T.  Then one lane per candidate (g, d), d = 0 .. Lmax-1: per live
 * candidate one read-only probe of the map's table and one probe of the observation set with two 64-bit atomics (a
 * compare-and-swap and a min), 4 B of set position per candidate, two more passes over those 4 B: proportional to
 * T x Lmax.  Per created pair 12 B of log, an exchange and an add on its entry.  Only in a growth is anything proportional
 * to E: when 2 (E + B) exceeds the set's slots a set of the next sufficient power of two is made and every old slot
 * re-inserted (`rehashes` counts these); the log grows geometrically by device copies.  Three host waits per call: T, the
 * totals, the end.  sdm_vmap_fetch_cameras: one lane per requested entry walks and sorts its list (insertion, quadratic
 * in the list's length); two host waits: the total, the end.
 * Memory: 20 B per set slot (at least 2 (E + B) slots, so at least 40 B per pair of the bound), 12 B per log entry of
 * capacity (at least E + B), 8 B per record of capacity, allocated at the first observe.
 * Limits: set and log are sized a priori by B, which counts every candidate as new -- a block observed by many
 * neighbours reserves far more than it creates -- and they never shrink before sdm_vmap_close (sdm_vmap_clear keeps the
 * capacity); the lists go stale with sdm_set_pose exactly as the stored xyz do (remedy: sdm_vmap_clear, integrate and
 * observe the resident slots again); an observation cannot be removed: removing one and shrinking the camera lists on
 * the persistent map remain later work; one rank only per log: the logs of several ranks merge through
 * sdm_vmap_import_observations (below).  sdm_vmap_repose (below) carries the log through its id map when the poses
 * move.  sdm_vmap_retire (below) is that later work: it removes the observations of a set of keyframes and shortens the
 * camera lists. */
typedef struct {
    long long plain_total;     /* out: T */
    long long unmapped;        /* out: plain points without an entry */
    long long candidates;      /* out: sum of |C(g)| over the mapped points */
    long long first_created;   /* out: E before the call */
    long long created;         /* out */
} sdm_vmap_observe_delta;
typedef struct {
    unsigned *entry;           /* [capacity] or NULL */
    int *tag;                  /* [capacity] or NULL */
    long long capacity;
    int on_device;             /* pointers are device memory of this context's GPU, 4-byte aligned */
} sdm_vmap_observations;
typedef struct {
    long long *cam_offsets;    /* [capacity + 1] or NULL */
    int *cam_tags;             /* [cam_capacity] or NULL */
    long long capacity;        /* in: entries cam_offsets serves; count must not exceed it */
    long long cam_capacity;    /* in */
    int on_device;             /* pointers (and ids) are device memory: cam_offsets 8-byte, cam_tags and ids 4-byte aligned */
    long long cam_total;       /* out: sum of the requested lists' lengths */
} sdm_vmap_cameras;
typedef struct {
    long long observations;    /* E */
    long long calls;           /* successful sdm_vmap_observe and sdm_vmap_import_observations calls since open / clear */
    long long table_slots;     /* slots of the observation set */
    long long rehashes;        /* its growths since open / clear */
} sdm_vmap_obs_info;
int sdm_vmap_observe(sdm_ctx *ctx, int n, const int *slots, const int *tags /*[n] or NULL*/, int n_nbr,
                     const int *nbr_slots /*[n][n_nbr] or NULL*/, const int *nbr_tags /*[n][n_nbr] or NULL*/, int source,
                     double max_sigma, double min_rho, sdm_vmap_observe_delta *ob);
int sdm_vmap_get_obs_info(sdm_ctx *ctx, sdm_vmap_obs_info *info);
int sdm_vmap_fetch_observations(sdm_ctx *ctx, long long first, long long count, sdm_vmap_observations *out);
int sdm_vmap_fetch_cameras(sdm_ctx *ctx, const unsigned *ids /*[count] or NULL*/, long long first, long long count,
                           sdm_vmap_cameras *cams);
/* Classification on the persistent map: a rule over the per-entry state decides on the device which entries are surface,
 * every entry keeps a persistent `published` flag, and every sdm_vmap_classify reports exactly which ids became accepted
 * (the consumer emits `new point` for them) and which were retracted (`del point`).  The recipe is: integrate a block,
 * observe it, carve it, classify; only the delta crosses the link.  Nothing in the reference does this; the semantics
 * below are this library's (tests/vmap_class_np.py restates them in NumPy).  Requires an open map.
 *   - State: every entry carries `published`, one byte, 0 or 1.  It is 0 when the entry is created and 0 after
 *     sdm_vmap_clear; it survives table rehashes and record growth; sdm_vmap_close and sdm_destroy free it.  No other
 *     call reads or writes it.  Classification removes nothing from the map: it only labels entries.
 *   - Inputs of entry id: the multiplicity and the stored sigma of its record; ncam, the length of its observation list
 *     (0 if no sdm_vmap_observe has run); crossings and ends (both 0 if no sdm_vmap_carve has run).
 *   - Rule (sdm_vmap_rule, plain integers and one float).  The LOCAL tests pass iff all of
 *         multiplicity >= min_multiplicity,  ncam >= min_cameras,  ends >= min_ends,
 *         crossings * ratio_den <= ends * ratio_num,  key(sigma) <= key(max_sigma)
 *     hold.  The ratio test compares the exact integer products (128 bits on the device; nothing wraps).  key() is
 *     sdm_extract_points_voxel's total order on float bit patterns (negatives, -0, +0, positives, +Inf, then the NaNs
 *     with the sign bit clear; NaNs with the sign bit set come first): every pattern has a place, so a NaN max_sigma is a
 *     defined threshold.  Every compare is an integer compare: the result has no rounding.
 *   - NEIGHBOUR test: nb(id) = the number of the 26 cells adjacent (Chebyshev distance 1) to the entry's cell that hold an
 *     entry whose LOCAL tests pass.  A cell with a coordinate outside [-2^20, 2^20) holds nothing.  The entry's cell is
 *     floorf(xyz_k * inv) of its record, as sdm_vmap_integrate forms it.
 *   - passing(id) = LOCAL && nb(id) >= min_neighbours.  min_neighbours == 0 makes no neighbour probe.  passing does not
 *     depend on published: it is a pure function of the map, the evidence, the log and the rule.
 *   - Delta (sdm_vmap_class_delta): examined = M; accepted = entries with passing && !published; retracted = entries with
 *     !passing && published; accepted_ids and retracted_ids list those ids in ascending order; published_total = entries
 *     published after the call.  commit != 0: the listed entries flip their flag.  commit == 0: the lists and counts are
 *     returned and no state changes (published_total is then the count before the call).  The id pointers follow
 *     on_device (4-byte aligned there); either may be NULL, which gives counts only, and its capacity is then ignored.
 *   - Capacity: accepted > accepted_capacity with accepted_ids != NULL is SDM_EINVAL, and so is retracted >
 *     retracted_capacity with retracted_ids != NULL: the counts are filled, neither array is written and no flag changes
 *     (sdm_voxel_cameras' cam_total > cam_capacity contract).  The caller sizes the arrays and calls again.
 *   - Invariants.  C1: after a committing call, classifying again with the same rule and an unchanged map gives
 *     accepted = retracted = 0.  C2: with rules A then B, both committing, B's accepted_ids = {passing_B \ passing_A} and its
 *     retracted_ids = {passing_A \ passing_B}.  C3: the flags after any sequence of committing calls equal passing under
 *     the last rule; entries created after that call read 0.  C4: a call changes no record, id, evidence counter or
 *     observation, no field of sdm_vmap_get_info or sdm_vmap_get_obs_info, and no plane, flag, list or counter of the
 *     engine.  C5: every output is bitwise the same from run to run, whatever the table layout.
 * sdm_vmap_fetch_published returns the flags as u8 for entries first .. first + count - 1 (ids == NULL) or ids[0 .. count)
 * (first must be 0; ids and out follow on_device, ids 4-byte aligned there), count <= capacity; zeros before the first
 * classify.  sdm_vmap_get_class_info: published = entries whose flag is set, calls = committing sdm_vmap_classify calls
 * since open / clear.
 * Errors, all raised before any flag changes (a refused call leaves every info and every full fetch as it was):
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: NULL ctx, rule or delta; ratio_den == 0; min_neighbours outside 0 .. 26; a negative capacity; a misaligned
 *     device pointer; the capacity case above; the fetch errors exactly as sdm_vmap_fetch's (count < 0, count > capacity, a
 *     range beyond M, an id >= M, first != 0 with ids, a misaligned device pointer, no destination).
 *   SDM_EHIP: an allocation failure -- everything is allocated before anything is written.
 * On an argument or state refusal the outs of the delta are 0; in the capacity case all four are filled (published_total
 * with the count before the call).
 * Cost per sdm_vmap_classify: one pass over the M entries -- 4 B + 8 B + 4 B + 16 B + 1 B read and 1 B of scratch written
 * per entry -- then, with min_neighbours > 0, per LOCAL-passing entry 12 B of xyz and up to 26 read-only probes of the
 * table (8 B keys; on a hit 4 B of id and 1 B of scratch), ended early once min_neighbours is reached; two scans over
 * M / 2048 tile counts; one more pass over 2 B per entry that writes 4 B per listed id.  The pass is O(M) per call, not
 * O(block), and the probes make it latency-bound.  One host wait for the counts, one for the end; with host id lists
 * 4 B per listed id cross the link, and nothing else does.
 * Memory: 1 B per record of capacity, allocated at the first classify, plus 1 B per entry of per-call scratch.
 * Limits: the pass is O(M) per call on the device; there is no hysteresis -- an entry whose evidence hovers at a threshold
 * is accepted and retracted again and again, and damping that is the consumer's; the flags go stale with sdm_set_pose
 * exactly as the evidence does (remedy: sdm_vmap_clear, then integrate, observe, carve and classify the resident slots
 * again); one rank only: the flags do not travel with sdm_vmap_import (below) -- classify the merged map.
 * sdm_vmap_repose (below) carries or restarts the flags when the poses move. */
typedef struct {
    unsigned min_multiplicity;
    unsigned min_cameras;
    unsigned long long min_ends;
    unsigned ratio_num;          /* crossings * ratio_den <= ends * ratio_num */
    unsigned ratio_den;          /* >= 1 */
    float max_sigma;             /* compared under key(); any bit pattern */
    int min_neighbours;          /* 0 .. 26; 0: no neighbour probe */
} sdm_vmap_rule;
typedef struct {
    unsigned *accepted_ids;        /* in: [accepted_capacity] or NULL */
    unsigned *retracted_ids;       /* in: [retracted_capacity] or NULL */
    long long accepted_capacity;   /* in */
    long long retracted_capacity;  /* in */
    int on_device;                 /* in: 1: both id arrays are device memory of this context's GPU (4-byte aligned) */
    long long examined;            /* out: M */
    long long accepted;            /* out */
    long long retracted;           /* out */
    long long published_total;     /* out: entries published after the call */
} sdm_vmap_class_delta;
typedef struct {
    long long published;       /* entries whose flag is set */
    long long calls;           /* committing sdm_vmap_classify calls since open / clear */
} sdm_vmap_class_info;
typedef struct {
    unsigned char *published;  /* [capacity] */
    long long capacity;
    int on_device;             /* published (and ids) are device memory of this context's GPU (ids: 4-byte aligned) */
} sdm_vmap_published;
int sdm_vmap_classify(sdm_ctx *ctx, const sdm_vmap_rule *rule, int commit, sdm_vmap_class_delta *delta);
int sdm_vmap_get_class_info(sdm_ctx *ctx, sdm_vmap_class_info *info);
int sdm_vmap_fetch_published(sdm_ctx *ctx, const unsigned *ids /*[count] or NULL*/, long long first, long long count,
                             sdm_vmap_published *out);
/* Importing into the persistent map: sdm_vmap_fetch writes an entry's fields out, sdm_vmap_import reads them back in --
 * into ANY open map.  That is how the maps of several ranks become one, how a saved map is restored, and how a map is
 * re-binned at another voxel_size.  Nothing in the reference does this; the semantics below are this library's
 * (tests/vmap_import_np.py restates them in NumPy).  Requires an open map; voxel_size, inv, the cell floorf(xyz_k * inv),
 * mergeability and key(sigma) are sdm_vmap_integrate's, with the DESTINATION map's voxel_size.
 *   - Sources: `src` and `extra` are the two structs sdm_vmap_fetch writes, read here.  src->xyz and src->rho_sigma are
 *     required (count > 0); src->pixel, src->intensity and extra->tag may be NULL and then read as 0; extra->multiplicity
 *     NULL (or extra NULL) reads as 1 for every record; extra->epoch is ignored.  src->on_device covers every source
 *     pointer, aligned there as sdm_vmap_fetch asks (4 B; rho_sigma: 8 B).  src->capacity >= count.  The sources are only
 *     read.
 *   - Call number: the import is call number c of the map: `calls` counts successful sdm_vmap_integrate and
 *     sdm_vmap_import calls alike, from 1 since open or clear.
 *   - Importing: the records r = 0 .. R-1, R = count, with multiplicity m_r, are processed as if one by one in increasing r:
 *       * a record whose xyz is unmergeable or whose m_r is 0 adds 1 to `dropped`, is not stored, and gets
 *         dst_ids[r] = 0xFFFFFFFF;
 *       * a record whose voxel has no entry creates entry id = M from its copied bits: xyz, pixel, rho_sigma, intensity,
 *         tag, multiplicity = m_r, epoch = c; then M += 1;
 *       * otherwise multiplicity = min(2^32 - 1, multiplicity + m_r), and if key(sigma_r) < the key of the entry's stored
 *         sigma, STRICTLY, the record replaces the stored one (its five fields) and epoch = c.
 *     dst_ids[r] is the entry that holds record r's voxel after the call.  `points` adds the sum of m_r over the stored
 *     records (a 64-bit sum); the map's `dropped` adds the call's.
 *   - Delta (sdm_vmap_import_delta): total = R; dropped; first_created = M before the call; created = entries appended,
 *     with ids first_created .. first_created + created - 1 in the order of their first record; updated = entries with
 *     id < first_created whose epoch became c; updated_ids lists those in ascending order of the r of the entry's final
 *     winner in this call, as sdm_vmap_integrate orders by g.  dst_ids and updated_ids follow delta->on_device.
 *   - Invariants.  I1: importing a range in one call or in any split into consecutive calls leaves byte-identical maps
 *     except `epoch` and `calls`.  I2: with B a map built from the clouds Q and A a map of the same voxel_size built from
 *     the clouds P, importing the full sdm_vmap_fetch of B into A gives exactly the map of integrating P then Q into one
 *     map -- every field but `epoch`, `calls` and `dropped` ("smallest key(sigma) wins, ties to the earlier, ids by first
 *     appearance, multiplicities add saturating" is associative over consecutive groups).  I3: importing a map's own full
 *     fetch into an empty map of the same voxel_size reproduces it, ids included (dst_ids[r] = r; `points` is the sum of
 *     the fetched multiplicities, which is the source's `points` unless a multiplicity had saturated).
 * sdm_vmap_import_observations does the same for the log: pairs k = 0 .. P-1, P = count, are processed as if in
 * increasing k.  The pair's entry is entry[k], or entry_map[entry[k]] when entry_map != NULL (an entry[k] >= map_count
 * is rejected): pass a source rank's log with sdm_vmap_import's dst_ids as the map and no host gather is needed -- the
 * dropped records' 0xFFFFFFFF falls out by itself.  A pair whose resolved entry is >= M or whose tag is < 0 adds 1 to
 * `rejected` and contributes nothing: a count, like `unmapped` in sdm_vmap_observe, never a refusal.  A pair not yet
 * stored is appended at index E; then E += 1.  Outs: total = P, rejected, first_created = E before the call, created.
 * Invariants: any split into consecutive calls leaves the same log; importing the same pairs again creates nothing; every
 * entry's camera list is independent of the order of the calls.  The map itself is only read.  sdm_vmap_get_obs_info's
 * `calls` counts these calls too.
 * Everything is integer or copied bits: every returned array is bitwise the same from run to run.
 * Errors, all raised before the map or the log changes (a refused call leaves both infos, a full fetch and the log as
 * they were; no refusal depends on device data):
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: a NULL ctx, src or io; count < 0; count > src->capacity; a NULL xyz, rho_sigma, entry or tag with
 *     count > 0; a misaligned device pointer; updated_ids != NULL with updated_capacity < min(M, R), the a-priori bound on
 *     `updated` (total and first_created are filled), or < 0; M + R > 2^30; map_count < 0; E + P > 2^30 (the bound of
 *     sdm_vmap_observe's B).
 *   SDM_EHIP: an allocation failure while growing -- growth is done before anything is inserted.
 * On an argument or state refusal the outs are 0, except total and first_created once known.
 * Changes no plane, flag, list or counter of the engine; evidence counters, observations and published flags of the
 * existing entries survive the growth an import forces, and a created entry's read 0.
 * Cost per sdm_vmap_import, outside a growth proportional to R: host sources are staged through the map's scratch (33 B
 * per record with every field); per record 24 B read, one probe of the table with four integer atomics (a 64-bit
 * compare-and-swap, a 64-bit min, a 32-bit min and a 32-bit compare-and-swap loop that adds m_r and clamps at 2^32 - 1,
 * so the per-call count stays 32 bits and a table slot 28 B) and 4 B of table position; three more passes over those 4 B
 * and the table fields; 4 B of dst_ids per record and a 37 B record per created or updated entry.  Two host waits: the
 * counts, the end.  Per sdm_vmap_import_observations: 8 B per pair read (12 B with a map), one probe of the set with a
 * 64-bit compare-and-swap and a 64-bit min, two more passes over 4 B per pair; per created pair a 12 B log entry.  The
 * tags of device pairs are copied back once (4 B per pair) to keep sdm_vmap_fetch_cameras' bound on a list's length: every
 * tag >= 0 of a call counts as a distinct tag observed for that refusal, a rejected pair's too, so the bound can only be
 * larger than the longest list.
 * Two host waits.  Set and log are sized a priori for E + P.
 * Limits: evidence counters and published flags do not travel: sdm_vmap_carve and sdm_vmap_classify run on the merged
 * map, and evidence carved on one rank is relative to that rank's entries, so it does not add up across ranks; the
 * records of several ranks reach one context through host or device buffers the caller moves -- there is no collective
 * inside the call; a record cannot be removed by an import (sdm_vmap_retire, below, removes the records of retired
 * keyframes). */
typedef struct {
    unsigned *dst_ids;            /* in: [count] or NULL; out: entry id of record r, 0xFFFFFFFF for a dropped one */
    unsigned *updated_ids;        /* in: [updated_capacity] or NULL */
    long long updated_capacity;   /* in */
    int on_device;                /* in: 1: dst_ids and updated_ids are device memory (4-byte aligned) */
    long long total;              /* out: R = count */
    long long dropped, first_created, created, updated;   /* out */
} sdm_vmap_import_delta;
int sdm_vmap_import(sdm_ctx *ctx, const sdm_point_buffers *src, const sdm_vmap_fields *extra /* or NULL */,
                    long long count, sdm_vmap_import_delta *delta /* or NULL */);
typedef struct {
    const unsigned *entry;        /* [count] */
    const int *tag;               /* [count] */
    const unsigned *entry_map;    /* [map_count] or NULL: the pair's entry is entry_map[entry[k]] */
    long long map_count;
    int on_device;                /* all three pointers, 4-byte aligned */
    long long total, rejected, first_created, created;    /* out */
} sdm_vmap_obs_import;
int sdm_vmap_import_observations(sdm_ctx *ctx, long long count, sdm_vmap_obs_import *io);
/* Re-placing the persistent map under new keyframe poses: bundle adjustment and loop closing move poses long after the
 * slots of the keyframes that built the map were recycled, and the four limits above all end in "clear and integrate the
 * resident slots again".  An entry's record holds what its xyz was computed from -- the winning point's pixel, its rho and
 * the keyframe's tag -- so sdm_vmap_repose recomputes every entry's xyz on the device from a table of (tag, K, Tcw),
 * bins the entries again and carries the observation log, the counters and the flags through the id map.  Nothing in
 * the reference does this; the semantics are this library's (tests/vmap_repose_np.py restates them in NumPy).  Requires an
 * open map.  tags[n_poses], K[n_poses][4] = {fx, fy, cx, cy} and Tcw[n_poses][12] are host arrays; K is passed because the
 * slot of an old keyframe is long gone.
 *   - New xyz of old entry i: if the record's tag equals tags[p], xyz becomes exactly what UpdateSemiDensePointSet's
 *     arithmetic (sdm_pointset) gives for K[p], Tcw[p], x = pixel & 0xffff, y = pixel >> 16 and the record's rho -- the same
 *     device function, no FMA, (double)rho < 1e-6 -> (0, 0, 0) included; the 2-pixel inset plays no part.  An entry whose
 *     tag is not in the table keeps its xyz bits.  A non-finite pose is no error: it yields non-finite xyz.
 *   - Re-binning: the result is defined as if the old entries i = 0 .. M-1 were imported by sdm_vmap_import, in increasing
 *     i, into an empty map of the same voxel_size, record i carrying its new xyz, its pixel, rho_sigma, intensity and tag
 *     and m_i = its multiplicity: a record whose new xyz is unmergeable is dropped; new ids are the order of first
 *     appearance, so survivors keep their relative order; within a voxel the smallest key(sigma) wins and a tie goes to
 *     the lower old id; multiplicities add and saturate at 2^32 - 1.  One difference: the surviving record keeps its OLD
 *     epoch.  remap[i] is the entry that holds old entry i's voxel after the call, 0xFFFFFFFF for a dropped one.
 *   - Map info: calls += 1 (the call takes a call number, though no epoch becomes it); voxels = the new M; points, dropped,
 *     table_slots and rehashes are unchanged (the table never shrinks; the new M is at most the old).
 *   - Observation log: rebuilt as if the old log, in log order, were passed to sdm_vmap_import_observations with
 *     entry_map = remap into an empty log: pairs of dropped entries vanish, pairs that become equal collapse, the
 *     survivors keep their relative order.  The set's slots, its rehashes and the obs info's calls are unchanged.  If no
 *     observe or import of observations has stored a pair, nothing is allocated or touched.
 *   - Evidence and published flags: with carry == 0 both counters and the flag are 0 for every new entry (they restart);
 *     with carry == 1 a new entry's crossings and ends are the 64-bit sums over the old entries mapped to it and its flag
 *     the OR of theirs.  The class info's `published` follows the flags; its calls is unchanged.
 *   - n_poses == 0 (NULL arrays allowed) is the identity on the map, the ids, the camera lists and -- with carry == 1 --
 *     evidence and flags: remap[i] = i.  Log indices may still be renumbered: the rebuilt log keeps the relative order
 *     of the surviving pairs.
 *   - Delta (sdm_vmap_repose_delta): examined = M before; reposed = entries whose tag is in the table; moved = of those,
 *     entries whose xyz changed in at least one bit; dropped; voxels = M after; merged = examined - dropped - voxels;
 *     observations_before and observations = E before and after.  remap follows delta->on_device.
 * Everything is copied bits, integer reductions, or the one float formula per entry: every output is bitwise the same from
 * run to run, whatever the table layout.
 * Errors, all raised before anything changes (a refused call leaves all four infos, a full fetch, the log, the evidence
 * and the flags as they were; no refusal depends on device data):
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: a NULL ctx or delta; n_poses < 0; a NULL tags, K or Tcw with n_poses > 0; a tag outside [0, 2^31); a tag
 *     listed twice; carry not 0 or 1; a misaligned device remap; remap != NULL with remap_capacity < M (examined is filled).
 *   SDM_EHIP: an allocation failure -- everything is allocated before anything is written.
 * On an argument or state refusal the outs are 0, except examined once known.
 * Changes no plane, flag, list or counter of the engine outside the map.
 * Cost: the pose table (84 B per pose, sorted by tag on the host) is uploaded once; per old entry one binary search and
 * 29 B read, 12 B of scratch xyz written; then one sdm_vmap_import of M device records into the emptied table (its cost
 * above, without the staging), 4 B of remap and a 37 B record per new entry; with carry 17 B read per old entry and up to
 * two 64-bit atomic adds and a byte; one pass over the new flags; one sdm_vmap_import_observations of the E old pairs
 * through remap, in place.  Two memsets over the table and the set.  Two host waits: the counts, the end; 4 B per old
 * entry cross the link for a host remap and nothing else does.  Measured: DESIGN.md s.22.
 * Memory: the peak extra is one second set of records (37 B per record of capacity) plus 16 B per old entry of scratch
 * (xyz, table position), 4 B more for a remap that is not a device buffer of the caller's, and with carry a second set
 * of counters and flags (17 B per record of capacity); the old sets are freed before the call returns.  The log and the
 * set are rebuilt in their own storage with 4 B per old pair of scratch.
 * Limits: only each voxel's winning point is re-placed -- the points that lost are gone, so a reposed map is not the map
 * of integrating everything again under the new poses; carried evidence belongs to rays walked under the old poses
 * (sdm_vmap_recarve, further below, walks the log's rays again under the new ones); two
 * successive reposes are not one repose with the union table (entries merged by the first stay merged); ids and log
 * indices change and remap is the consumer's only bridge; one rank only per map. */
typedef struct {
    unsigned *remap;              /* in: [remap_capacity] or NULL; out: new id of old entry i, 0xFFFFFFFF if dropped */
    long long remap_capacity;     /* in: >= M before the call when remap != NULL */
    int on_device;                /* in: 1: remap is device memory of this context's GPU (4-byte aligned) */
    int carry;                    /* in: 0: evidence counters and published flags restart at 0; 1: carried (above) */
    long long examined;           /* out: M before the call */
    long long reposed, moved, dropped, merged;   /* out */
    long long voxels;             /* out: M after the call */
    long long observations_before, observations;   /* out: E before / after */
} sdm_vmap_repose_delta;
int sdm_vmap_repose(sdm_ctx *ctx, int n_poses, const int *tags /*[n_poses]*/, const float *K /*[n_poses][4]*/,
                    const float *Tcw /*[n_poses][12]*/, sdm_vmap_repose_delta *delta);
/* Retiring keyframes from the persistent map: ORB-SLAM culls keyframes all the time, the reference skips the semi-dense
 * points of a bad keyframe, and its transcript has "del observation" next to "del point".  sdm_vmap_retire removes a set R
 * of keyframe tags from the map on the device and reports exactly what a consumer has to delete.  The semantics are this
 * library's (tests/vmap_retire_np.py restates them in NumPy).  Requires an open map.  tags[n_tags] is a host array; the old
 * entries are i = 0 .. M-1 and the old log pairs k = 0 .. E-1.
 *   - Pairs: a pair (entry, tag) is retired iff tag is in R.
 *   - Survivors.  mode SDM_VMAP_RETIRE_WINNER: entry i survives iff its record's tag is not in R (the reference's
 *     behaviour: the points of a bad keyframe disappear).  mode SDM_VMAP_RETIRE_UNOBSERVED: entry i survives iff at least
 *     one of its pairs is not retired -- a voxel lives as long as a live keyframe saw it.  This mode presupposes the recipe
 *     "integrate, then observe" per block: an entry that was never observed does not survive, and with E == 0 the map
 *     empties.  orphaned counts the survivors whose record's tag is in R (possible in mode UNOBSERVED only); their record
 *     stays bit for bit, retired tag included, because the points that lost are gone.
 *   - Map: new id = rank of i among the survivors, so survivors keep their relative order; every field of a survivor's
 *     record (xyz, pixel, rho_sigma, intensity, tag, multiplicity, epoch) is copied bits.  remap[i] is the new id, or
 *     0xFFFFFFFF for a dropped entry.  Map info: calls += 1; voxels = the new M; points, dropped, table_slots and rehashes
 *     are unchanged (the table never shrinks).  After the call exactly the survivors' voxels are found, under their new ids.
 *   - Log: the new log is the old log, in log order, without the retired pairs and without the pairs of dropped entries,
 *     entry ids through remap.  Nothing collapses (survivors are distinct).  Chains, list lengths, the set and
 *     sdm_vmap_fetch_cameras follow; the obs info's calls, slots and rehashes are unchanged.  removed counts the retired
 *     pairs on SURVIVING entries, listed with OLD entry ids in old log order; the pairs that vanish with a dropped entry are
 *     observations_before - observations - removed and are not listed ("del point" covers them).  If no pair was ever
 *     stored, nothing of the log is allocated or touched.
 *   - Evidence and published flags: with carry == 1 a survivor keeps its two counters and its flag; with carry == 0 all
 *     restart at 0.  The class info's `published` follows; its calls is unchanged.
 *   - Lists for the consumer: dropped_ids holds OLD ids, ascending, and dropped_published their flag before the call -- emit
 *     "del point" for those with flag 1; removed_entry / removed_tag are for "del observation"; then apply remap.
 *     dropped_published needs dropped_ids and removed_tag needs removed_entry (they share the capacity).
 *   - commit == 0: every out and every list is computed and nothing in the context changes (as sdm_vmap_classify).
 *   - n_tags == 0 (NULL tags allowed) is the identity in mode WINNER: remap[i] = i; with carry == 0 evidence and flags
 *     restart, as in sdm_vmap_repose.  (In mode UNOBSERVED the never-observed entries still go.)
 *   - No memory of R: a later integrate, observe or import with a retired tag is accepted as before.
 * Everything is copied bits and integer scans: every output is bitwise the same from run to run, whatever the table
 * layout.
 * Errors, all raised before anything changes (a refused call leaves all four infos, a full fetch, the log, the camera
 * lists, the evidence and the flags as they were):
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: a NULL ctx or delta; n_tags < 0; NULL tags with n_tags > 0; a tag outside [0, 2^31); a tag listed twice;
 *     mode, carry or commit not 0 or 1; a negative capacity of a given array; a misaligned device pointer;
 *     dropped_published without dropped_ids or removed_tag without removed_entry; a capacity smaller than the count it has
 *     to hold (remap_capacity < M, dropped_capacity < dropped, removed_capacity < removed, with a non-NULL array): all
 *     counts are filled, no array is written, nothing changes -- size the arrays and call again.  The counts come from a
 *     read-only marking phase that ends in the first host wait.
 *   SDM_EHIP: an allocation failure -- everything is allocated before anything is written.
 * On an argument or state refusal the outs are 0, except examined and observations_before once known.
 * Changes no plane, flag, list or counter of the engine outside the map.
 * Cost: R is sorted on the host and uploaded once (4 B per tag).  Marking: per old pair two passes (8 B read, one binary
 * search, 1 B mark), per old entry one binary search and 6 B read, then tile counts and four scans.  Lists: one pass over
 * the entry marks (4 B of remap per old entry, 5 B per dropped entry), one over the pair marks (8 B per removed pair).
 * Commit: one 37 B record copied per survivor (with carry 17 B more), two memsets over the table and one key computed
 * and inserted per survivor; two memsets over the set and the chains and one sdm_vmap_import_observations of the E old
 * pairs through remap, in place.  Two host waits: the counts, the end.  For host lists 4 B per old entry, 5 B per dropped
 * entry and 8 B per removed pair cross the link; with device lists nothing but R does.  Measured: DESIGN.md s.23.
 * Memory: the peak extra is one second set of records (37 B per record of capacity), 2 B per old entry and 1 B per old
 * pair of marks, 4 B per old entry for a remap that is not a device buffer of the caller's, the staging of host lists, and
 * with carry a second set of counters and flags (17 B per record of capacity); the old sets are freed before the call
 * returns.  The log and the set are rebuilt in their own storage with 4 B per old pair of scratch.  Table, set, log and
 * records keep their capacity.
 * Limits: the points that lost are gone -- a map after WINNER-retiring R is a subset of the map of integrating only the
 * other keyframes, not equal to it; the multiplicity is NOT reduced, because the map does not know which keyframe added
 * what; carried counters still contain the rays of retired keyframes; ids and log indices change and remap is the
 * consumer's only bridge; one rank only per map; the evidence without the retired rays is rebuilt from the log's pairs by
 * sdm_vmap_recarve (next). */
#define SDM_VMAP_RETIRE_WINNER 0
#define SDM_VMAP_RETIRE_UNOBSERVED 1
typedef struct {
    /* in */
    int mode;                      /* SDM_VMAP_RETIRE_WINNER (0) or SDM_VMAP_RETIRE_UNOBSERVED (1) */
    int carry;                     /* 0: evidence counters and published flags restart at 0; 1: survivors keep theirs */
    int on_device;                 /* 1: every array below is device memory of this context's GPU (4-byte aligned; u8: any) */
    unsigned *remap;               /* [remap_capacity] or NULL: new id of old entry i, 0xFFFFFFFF if dropped */
    long long remap_capacity;
    unsigned *dropped_ids;         /* [dropped_capacity] or NULL: OLD ids of the dropped entries, ascending */
    unsigned char *dropped_published; /* [dropped_capacity] or NULL: their published flag before the call */
    long long dropped_capacity;
    unsigned *removed_entry;       /* [removed_capacity] or NULL: OLD entry id of each removed pair on a SURVIVING entry, in old log order */
    int *removed_tag;              /* [removed_capacity] or NULL */
    long long removed_capacity;
    /* out */
    long long examined;            /* M before */
    long long dropped, dropped_were_published, orphaned;
    long long voxels;              /* M after */
    long long observations_before, observations, removed;
    long long published_total;     /* after the call */
} sdm_vmap_retire_delta;
int sdm_vmap_retire(sdm_ctx *ctx, int n_tags, const int *tags /*[n_tags], host*/, int commit, sdm_vmap_retire_delta *delta);
/* Rebuilding the free-space evidence from the observation log: sdm_vmap_carve reads the resident slots of a block, so once
 * a repose has restarted (or carried) the counters, or a retire has kept the rays of retired keyframes in them, the evidence
 * of everything older than the last block could not be made again.  The map holds what that takes: the log's (entry, tag)
 * pairs are the rays, the entry's record holds the end point -- already re-placed by a repose -- and the caller holds the
 * poses, the table it hands to the repose.  sdm_vmap_recarve walks one ray per pair of the log through the map's table on
 * the device and adds to the per-entry counters.  It closes the online recipe: repose, (retire,) recarve, classify.  The
 * semantics are this library's (tests/vmap_recarve_np.py restates them with tests/vmap_carve_np.py's walker).  Requires an
 * open map.  tags[n_poses] and Tcw[n_poses][12] are host arrays; the log's pairs are k = 0 .. E-1.
 *   - Rays: pair k of the range first .. first + count - 1 (count == -1: to the end of the log) is (e, t) = (obs_entry[k],
 *     obs_tag[k]).  If t is not in tags, the pair adds 1 to pairs_unposed and nothing else.  Otherwise it is one ray from O
 *     to P: O is the camera centre of Tcw[p], tags[p] == t, formed on the host exactly as
 *     sdm_extract_points_voxel_freespace forms it -- Rwc[i][j] = Tcw[j*4+i], Ow_i = (Rwc[i][0]*t0 + Rwc[i][1]*t1) +
 *     Rwc[i][2]*t2, O = -Ow (tests/carve_np.camera_centre) -- and P is the xyz of record e as it stands now.
 *   - Walk: the skip rule, the cells, the integer-driven walk of exactly N steps, the tie rule and the counted cells
 *     s <= N - 1 - end_margin are sdm_extract_points_voxel_freespace's and sdm_vmap_carve's, word for word, with the map's
 *     voxel_size and inv; IEEE binary32, no FMA, the plain division.  A non-finite pose is not an error: its rays are
 *     skipped (rays_skipped), as is a ray with a cell outside [-2^20, 2^20) or with N > max_steps.
 *   - Counting: every counted cell whose key has an entry adds 1 to crossings[id]; the end cell is probed once and its
 *     entry gets 1 on ends[id], whatever end_margin.
 *   - State: the map, the log, the flags and every info struct are left as they are.  The counters are allocated and
 *     zeroed if no carve has run yet (the allocation of the first sdm_vmap_carve; it grows with the records as before).
 *     With reset == 1 both counters of all M entries are put to 0 before anything is added, also when the range or the
 *     table is empty; with reset == 0 the call adds to what is there.  No log (E == 0) is not an error: zero pairs.
 *   - Outs: pairs_total = pairs examined; pairs_unposed; rays_total = pairs_total - pairs_unposed; rays_skipped;
 *     cells_visited = counted (ray, cell) pairs; cells_hit = the sum of the crossings added; ends_hit = the sum of the
 *     ends added.
 * Consequences: with reset == 1 over the whole log the counters are a pure function of (records, log, table), bitwise --
 * unlike sdm_vmap_carve, whose evidence depends on which entries existed at each call.  The call is additive over any
 * split of the log range into calls with reset == 0.  P lies in its own entry's voxel, so every walked ray ends in an
 * entry: ends_hit == rays_total - rays_skipped, and ends[e] is the number of walked pairs of entry e.  Everything is an
 * integer sum: bitwise the same from run to run, whatever the table layout.
 * Errors, all raised before any counter changes; none depends on device data:
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: a NULL ctx or rc; n_poses < 0; a NULL tags or Tcw with n_poses > 0; a tag outside [0, 2^31); a tag listed
 *     twice; end_margin < 0; max_steps outside 1 .. SDM_FREESPACE_MAX_STEPS; reset not 0 or 1; first < 0, count < -1 or
 *     first + count > E.
 *   SDM_EHIP: an allocation failure -- everything is allocated before anything is written.
 * On a refusal the outs are 0.
 * Cost: the table of (tag, centre) is sorted by tag on the host and uploaded once, 20 B per pose.  One lane per pair: 8 B
 * of the log read and one binary search; a posed lane reads 12 B of the record's xyz and walks as sdm_vmap_carve does --
 * six float divisions, per counted cell one read-only probe of the table (on a hit one 64-bit atomic add), one probe for
 * the end cell.  With reset one memset over the counters.  One host wait: the end, with the totals; nothing but the table
 * and 48 B of totals crosses the link.  Log order is point-major, so a wave mixes cameras (a tag-sorted order has not been
 * measured).  Measured: DESIGN.md s.25.  Memory: 16 B per record of capacity if no carve has run, 20 B per pose of scratch.
 * Limits: one ray per distinct (entry, tag), not one per plain point as in sdm_vmap_carve -- the two agree only where
 * every multiplicity is 1; the ray ends at the voxel's WINNING point, not at each point the camera saw there; one rank
 * only (the counters do not travel: recarve on the merged map); recarving a range twice without reset counts twice. */
typedef struct {
    int end_margin;            /* in: >= 0 */
    int max_steps;             /* in: 1 .. SDM_FREESPACE_MAX_STEPS */
    int reset;                 /* in: 1: both counters of EVERY entry are set to 0 first; 0: the call adds to them */
    long long first, count;    /* in: the log pairs first .. first+count-1; count == -1: from first to the end of the log */
    long long pairs_total;     /* out: pairs examined */
    long long pairs_unposed;   /* out: of those, pairs whose tag is not in the table (no ray) */
    long long rays_total;      /* out: pairs_total - pairs_unposed */
    long long rays_skipped;    /* out */
    long long cells_visited;   /* out */
    long long cells_hit;       /* out: = sum of the crossings added */
    long long ends_hit;        /* out: = sum of the ends added */
} sdm_vmap_recarve_args;
int sdm_vmap_recarve(sdm_ctx *ctx, int n_poses, const int *tags /*[n_poses], host*/,
                     const float *Tcw /*[n_poses][12], host*/, sdm_vmap_recarve_args *rc);
/* Ray queries on the voxel map: every call above writes the map or lists its entries by id; these two ask it the spatial
 * question -- along this segment, which entry comes first?  sdm_vmap_cast_segments answers it for n caller-given segments,
 * sdm_vmap_render for one segment per pixel of a camera (K, Tcw) that lives in no slot: the view the map predicts for that
 * pose, the occlusion test of an (entry, camera) pair, the entry under a pixel.  The semantics are this library's
 * (tests/vmap_cast_np.py restates them).  Both require an open map and only read it.
 *   - Segment and walk: a ray is a segment from O to P, both float[3].  The cells cO, cP, the skip rule, N = sum_a |cP_a -
 *     cO_a|, step, r, tMax, tDel, the axis choice with its tie rule and the update are
 *     sdm_extract_points_voxel_freespace's, word for word, with the map's voxel_size and inv; IEEE binary32, no FMA, the
 *     plain division.  A ray is SKIPPED if any of the six cells is outside [-2^20, 2^20) (every compare is false for a NaN)
 *     or if N > max_steps.  cur at index s is the ray's cell of index s, for s = 0 .. N: s = 0 is O's cell, s = N is P's.
 *   - Examined cells: start_margin <= s <= N - end_margin, in increasing s (none if start_margin > N - end_margin).
 *     end_margin = 0 examines the end cell.  sdm_vmap_carve's and sdm_vmap_recarve's end_margin = m counts the same cells
 *     as end_margin = m + 1 here.
 *   - Filter: an examined cell STOPS the ray iff its key has an entry id with multiplicity[id] >= min_multiplicity and,
 *     when require_published != 0, published[id] != 0 (if no classify has run every flag reads 0).  An entry that fails
 *     the filter is transparent: the ray goes on.
 *   - Per ray: the first stopping cell gives hit_id = its id and hit_step = its s; a walked ray without one gives hit_id =
 *     SDM_VMAP_NO_HIT and hit_step = 0; a skipped ray hit_id = SDM_VMAP_RAY_SKIPPED and hit_step = 0.  Ids stay below
 *     2^30, so the two codes collide with none.
 *   - Totals: rays_total; rays_skipped; rays_hit; cells_visited = the examined cells up to and including the stopping one,
 *     summed over the walked rays.
 * sdm_vmap_cast_segments: ray i is (origins[i], ends[i]).  origins, ends, hit_id and hit_step all follow args->on_device
 * (there: 4-byte aligned); hit_id and hit_step hold args->capacity >= n elements and either may be NULL, not both.  hit_rho
 * is ignored.  n == 0 is valid.
 * sdm_vmap_render: one ray per pixel, ray i = y * W + x from O to P(x, y).  K[4] = (fx, fy, cx, cy) and Tcw[12] are host
 * arrays.  O is the camera centre of Tcw, formed on the host exactly as sdm_vmap_recarve forms it; P(x, y) is the
 * back-projection of the pixel at inverse depth rho_far by the device function of the point-set pass -- what
 * sdm_vmap_repose gives an entry with that pixel, that rho and that pose.  hit_id, hit_step and hit_rho follow
 * args->on_device and hold args->capacity >= W * H elements; any may be NULL, not all three.  For a hit on entry id with
 * record xyz (X, Y, Z): z = ((Tcw[8]*X + Tcw[9]*Y) + Tcw[10]*Z) + Tcw[11] and hit_rho = 1.0f / z (no FMA, the plain
 * division); otherwise hit_rho = +0.0f.  The answer is voxel-level: the hit entry's stored point need not project into
 * that pixel, and hit_rho belongs to the stored point, not to the ray's crossing of the voxel (it is negative or infinite
 * if that point is not in front of the camera).  A non-finite pose is no error: its rays are skipped.
 *   - State: neither call changes the map, the log, the counters, the flags, any info struct, or any plane or list of the
 *     engine.  Everything returned is a pure function of the arguments, the records' cells and multiplicities (render:
 *     and xyz), and the flags: bitwise the same from run to run, whatever the table layout.
 * Errors, all raised on the host before anything is queued; the four outs are then 0:
 *   SDM_EINVAL: a NULL ctx or args.
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: n < 0 or n > 2^30 (render: W or H outside 1 .. 65535, or W * H > 2^30); NULL origins or ends with n > 0
 *     (render: NULL K or Tcw); no destination at all; capacity < n (render: < W * H); a misaligned device pointer;
 *     start_margin < 0 or end_margin < 0; max_steps outside 1 .. SDM_FREESPACE_MAX_STEPS; require_published not 0 or 1;
 *     render: rho_far NaN or (double)rho_far < 1e-6 (the back-projection would return the origin).
 *   SDM_EHIP: an allocation failure, raised before any launch.
 * Cost: one lane per ray, ray i on lane i (render: raster order).  Per ray 24 B of segment (render: none), six float
 * divisions, and per examined cell one read-only probe of the table as in sdm_vmap_carve, plus 4 B of multiplicity (and 1 B
 * of flag) per entry met; the loop leaves at the first stopping cell.  4 B per ray and requested output are written.  Host
 * sources and destinations pass through engine staging (24 B / 4 B per ray and field): one copy per field of exactly n
 * elements.  One host wait: the end, with 32 B of totals.  Measured: DESIGN.md s.26.
 * Limits: one rank only; the answer is per voxel, at the winning point -- no sub-voxel intersection, no normals; positions
 * go stale with sdm_set_pose exactly as the records do (sdm_vmap_repose re-places them). */
#define SDM_VMAP_NO_HIT 0xFFFFFFFFu
#define SDM_VMAP_RAY_SKIPPED 0xFFFFFFFEu
typedef struct {
    int start_margin;          /* in: >= 0; the first start_margin cells of the ray are not examined */
    int end_margin;            /* in: >= 0; the last end_margin cells are not examined (0: the end cell is) */
    int max_steps;             /* in: 1 .. SDM_FREESPACE_MAX_STEPS; a longer ray is skipped, not truncated */
    unsigned min_multiplicity; /* in: entries with fewer points are transparent */
    int require_published;     /* in: 0 or 1; 1: unpublished entries are transparent */
    int on_device;             /* in: the arrays below (and origins / ends) are device pointers */
    long long capacity;        /* in: elements each destination holds */
    unsigned *hit_id;          /* [capacity] or NULL */
    int *hit_step;             /* [capacity] or NULL */
    float *hit_rho;            /* [capacity] or NULL; sdm_vmap_render only */
    long long rays_total;      /* out */
    long long rays_skipped;    /* out */
    long long rays_hit;        /* out */
    long long cells_visited;   /* out */
} sdm_vmap_cast_args;
int sdm_vmap_cast_segments(sdm_ctx *ctx, long long n, const float *origins /*[n][3]*/, const float *ends /*[n][3]*/,
                           sdm_vmap_cast_args *args);
int sdm_vmap_render(sdm_ctx *ctx, const float *K /*[4], host*/, const float *Tcw /*[12], host*/, int W, int H, float rho_far,
                    sdm_vmap_cast_args *args);
/* Connected components of the voxel map's entries: every filter above is local -- one entry's counters, the occupancy of its
 * 26 adjacent cells -- and cannot see a small floating island; this call answers the global question: which entries belong
 * to a connected piece of at least k voxels, and which do not?  The semantics are this library's (tests/vmap_comp_np.py
 * restates them).  It requires an open map and only reads it.
 *   - Members: entry id is a MEMBER iff multiplicity[id] >= min_multiplicity and, when require_published != 0,
 *     published[id] != 0 (if no classify has run every flag reads 0): the filter of the ray queries above.
 *   - Cell: the cell of an entry is floorf(xyz_k * inv) of its record, as sdm_vmap_classify forms it.
 *   - Adjacency: two cells are adjacent iff they differ by an offset d in {-1, 0, 1}^3, d != 0, with |dx| + |dy| + |dz| <=
 *     1, 2, 3 for connectivity = 6, 18, 26.  A cell with a coordinate outside [-2^20, 2^20) holds nothing: the range test
 *     comes before the key is formed, so the last cell of one row is never taken for the first cell of the next.
 *   - Components: the classes of the transitive closure of "both members, cells adjacent".
 *   - Per entry (arrays of M elements, in id order): label[id] = the smallest id of its component; size[id] = the number
 *     of members of its component.  A non-member gets label SDM_VMAP_NO_COMPONENT and size 0.  Ids stay below 2^30, so the
 *     code collides with none.
 *   - Small list: with min_size > 0, small_ids is the ascending list of the members whose component has fewer than
 *     min_size members -- the ids a consumer drops, or emits a deletion for.  min_size == 0 lists nothing.
 *   - Totals: entries = M; members; components = the ids with label[id] == id; largest = the size of the largest
 *     component (0 without members); small = the length of the small list; small_components = the components it comes from.
 * label, size and small_ids follow args->on_device (there: 4-byte aligned).  label and size hold args->capacity >= M
 * elements, small_ids holds args->small_capacity.  Any of them may be NULL; all three NULL is valid and gives the totals
 * only.  M == 0 is valid and queues nothing.
 *   - Capacity: small > small_capacity with small_ids != NULL is SDM_EINVAL; the six totals are filled and no destination
 *     is written (sdm_vmap_classify's contract: counts first, one wait, and the writing launch is queued only if the call
 *     is not refused).  The caller sizes the array and calls again.
 *   - State: the call changes no record, id, evidence counter, flag or log entry, no field of any info struct, and no plane
 *     or list of the engine.  Every output is a pure function of the arguments, the records' cells and multiplicities, and
 *     the flags: bitwise the same from run to run, whatever the table layout and whatever order the device linked things in.
 * Errors, all raised on the host before anything is queued; the six totals are then 0:
 *   SDM_EINVAL: a NULL ctx or args.
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: connectivity not 6, 18 or 26; require_published not 0 or 1; a negative capacity or small_capacity;
 *     capacity < M with label or size given; a misaligned device pointer.
 *   SDM_EHIP: an allocation failure, raised before any launch.
 * Cost: one lane per entry.  A lock-free union-find over the map's own table: per member 12 B of record, 3, 9 or 13
 * read-only probes (each undirected pair of cells is met once) and per link found a walk of parent[] with path halving and
 * one compare-and-swap; then one walk and one 32-bit add per member, and two passes in tiles for the counts and the
 * writes.  Scratch: 8 B per entry.  Host destinations pass through engine staging: one copy per array of exactly M
 * (small_ids: small) elements.  Two host waits: the totals (40 B), then the end.  Measured: DESIGN.md s.27.
 * Limits: the pass is O(M) per call and not incremental; it is voxel-level -- the winning point's cell; it goes stale with
 * sdm_set_pose exactly as the records do (sdm_vmap_repose re-places them); there is no hysteresis; the flags are not
 * touched -- retracting a speckle is the consumer's business, or a later classify's; one rank only. */
#define SDM_VMAP_NO_COMPONENT 0xFFFFFFFFu
typedef struct {
    int connectivity;          /* in: 6, 18 or 26 */
    unsigned min_multiplicity; /* in: entries with fewer points are no members */
    int require_published;     /* in: 0 or 1; 1: unpublished entries are no members */
    unsigned min_size;         /* in: components of fewer members are small; 0: none is */
    int on_device;             /* in: the arrays below are device pointers */
    long long capacity;        /* in: elements label and size hold */
    long long small_capacity;  /* in: elements small_ids holds */
    unsigned *label;           /* [capacity] or NULL */
    unsigned *size;            /* [capacity] or NULL */
    unsigned *small_ids;       /* [small_capacity] or NULL */
    long long entries;         /* out: M */
    long long members;         /* out */
    long long components;      /* out */
    long long largest;         /* out */
    long long small;           /* out */
    long long small_components;/* out */
} sdm_vmap_comp_args;
int sdm_vmap_components(sdm_ctx *ctx, sdm_vmap_comp_args *args);
/* Per-entry surface normals and surface variation of the voxel map: for every entry of a range, the unit normal of the plane
 * through the stored points of the member entries in the (2r+1)^3 cells around it, the surface variation lambda_min /
 * (lambda_0 + lambda_1 + lambda_2), and how many points went in; optionally oriented towards the camera of the entry's
 * winning keyframe.  The semantics are this library's (tests/vmap_normals_np.py restates them) and are normative operation
 * by operation: every output is bitwise reproducible.  It requires an open map and only reads it.
 *   - Arithmetic: all of it is IEEE binary32: no fused multiply-add, the plain correctly rounded division and sqrtf,
 *     denormals kept.  Each product is rounded before the add or subtract that takes it.
 *   - Members: entry id is a MEMBER iff multiplicity[id] >= min_multiplicity and, when require_published != 0,
 *     published[id] != 0 (if no classify has run every flag reads 0): the member test of sdm_vmap_components, word for
 *     word.  The cell of an entry is c = floorf(P_k * inv) of its record point P, as sdm_vmap_components forms it.
 *   - Samples: a member id with record point P visits the offsets d in {-r..r}^3, r = radius, in lexicographic order, dx
 *     slowest and dz fastest; (0,0,0) is included and gives the entry itself.  A cell with a coordinate outside [-2^20,
 *     2^20) holds nothing: the range test comes before the key is formed.  The cell's entry j is a sample iff it exists
 *     and is a member.  Its coordinates are q_a = (xyz_j[a] - P[a]) * inv: one subtract, then one multiply.
 *   - Sums: all sums start at +0 and accumulate in visiting order: k += 1; s_a = s_a + q_a; m_ab = m_ab + q_a*q_b for
 *     (a,b) = (0,0),(0,1),(0,2),(1,1),(1,2),(2,2).  points[id - first] = k for a member and 0 for a non-member.
 *   - Covariance: if k < min_points the entry is not estimated.  Otherwise kf = (float)k; mu_a = s_a / kf;
 *     C_ab = m_ab / kf - mu_a*mu_b.
 *   - Eigen-solve: A = C (symmetric), V = I; a cyclic Jacobi of exactly 6 sweeps that uses only + - x / sqrt.  Each sweep
 *     takes the pairs (p,q) = (0,1), (0,2), (1,2) in that order; r is the third index.  If A_pq == 0 (-0 too) the pair does
 *     nothing.  Else theta = (A_qq - A_pp) / (2*A_pq); t = copysignf(1, theta) / (fabsf(theta) + sqrtf(theta*theta + 1));
 *     c = 1 / sqrtf(t*t + 1); s = t*c; h = t*A_pq; A_pp = A_pp - h; A_qq = A_qq + h; A_pq = +0; with x = A_rp, y = A_rq:
 *     A_rp = c*x - s*y, A_rq = s*x + c*y; for i = 0,1,2 with x = V_ip, y = V_iq: V_ip = c*x - s*y, V_iq = s*x + c*y.
 *     An overflowing theta*theta, or an infinite theta, gives t = +-0: the rotation is the identity and A_pq becomes 0;
 *     this is no special case in code.
 *   - Result: lambda_i = A_ii.  m = 0; if lambda_1 < lambda_m then m = 1; if lambda_2 < lambda_m then m = 2: ties go to
 *     the lower index.  sum = (lambda_0 + lambda_1) + lambda_2; if !(sum > 0) the entry is not estimated.  Otherwise the
 *     normal is column m of V, not renormalised, and variation = (lambda_m < 0 ? +0.0f : lambda_m) / sum.
 *   - Orientation: the pose table is sdm_vmap_recarve's -- same checks, same camera centre O = -(Rwc * tcw) formed on the
 *     host; n_poses == 0 is valid.  An estimated entry whose record tag is in the table is ORIENTED: d_a = O_a - P_a,
 *     dot = (n_0*d_0 + n_1*d_1) + n_2*d_2, and if dot < 0 every component is negated.  A NaN dot does not flip, and the
 *     entry still counts as oriented.  An estimated entry whose tag is absent keeps the sign the rotations left.
 *   - Not estimated or non-member: normal = (+0,+0,+0) and variation = -1.0f.
 *   - Range and destinations: the entries first .. first + count - 1 (count == -1: to M); outputs are indexed by
 *     id - first.  normal holds 3 x capacity floats, variation and points capacity elements each, capacity >= the size of
 *     the range; they follow args->on_device (there: 4-byte aligned).  Any of them may be NULL; all three NULL is valid
 *     and returns the totals only.  An empty range queues nothing.
 *   - Totals: entries = the size of the range; members, estimated and oriented are counted within the range.
 *   - State: the call changes nothing.  Every output is a pure function of the arguments, the records (xyz, multiplicity,
 *     tag) and the flags: bitwise the same from run to run, whatever the table layout and the slicing.
 * Errors, all raised on the host before anything is queued; the four totals are then 0:
 *   SDM_EINVAL: a NULL ctx or args.
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: radius not 1 or 2; min_points outside 3 .. (2*radius+1)^3; require_published not 0 or 1; first < 0,
 *     count < -1, or first + count > M; a negative capacity; capacity below the range with any destination given; a
 *     misaligned device pointer; the pose table's refusals: negative n_poses, NULL tags or Tcw with n_poses > 0, a tag
 *     outside [0, 2^31), a tag listed twice.
 *   SDM_EHIP: an allocation failure, raised before any launch.
 * Cost: one lane per entry of the range; 27 or 125 read-only probes, on a hit 4 B of multiplicity (+ 1 B of flag) and 12 B
 * of xyz; nine running sums and the Jacobi state in registers; no scratch per entry.  The pose table is uploaded once, 20 B
 * per pose.  Host destinations pass through engine staging: one copy per array.  One host wait: the end, with 32 B of
 * totals.  Measured: DESIGN.md s.28.
 * Limits: O(range x (2r+1)^3) probes per call, not incremental; built on each voxel's winning point only; it goes stale
 * with sdm_set_pose as the records do (sdm_vmap_repose re-places them); oriented by the winner's camera alone; one rank
 * only. */
typedef struct {
    int radius;                /* in: 1 or 2 */
    unsigned min_points;       /* in: 3 .. (2*radius+1)^3 */
    unsigned min_multiplicity; /* in: as sdm_vmap_components */
    int require_published;     /* in: 0 or 1 */
    int on_device;             /* in: the three arrays are device pointers (4-byte aligned) */
    long long first, count;    /* in: entries first .. first+count-1; count == -1: to M */
    long long capacity;        /* in: elements each destination holds (normal: x3) */
    float *normal;             /* [capacity][3] or NULL */
    float *variation;          /* [capacity] or NULL */
    unsigned *points;          /* [capacity] or NULL: the samples k of each entry */
    long long entries, members, estimated, oriented;   /* out */
} sdm_vmap_normal_args;
int sdm_vmap_normals(sdm_ctx *ctx, int n_poses, const int *tags /*[n_poses], host*/,
                     const float *Tcw /*[n_poses][12], host*/, sdm_vmap_normal_args *args);
/* A triangle mesh of the voxel map's entries, stitched on the device: every OWNER -- a member at the bottom of its run of
 * members along the dominant axis of its normal -- joins the local height field over its own cell: itself, the
 * representative of the next column along u, of the next along v, and of the diagonal one.  A triangle is three entry ids;
 * a consumer takes the vertex positions from the records (sdm_vmap_fetch).  The semantics are this library's
 * (tests/vmap_mesh_np.py restates them); every output is an integer decided by comparisons and bitwise reproducible.  It
 * requires an open map and only reads it.
 *   - Members: entry id is a MEMBER iff multiplicity[id] >= min_multiplicity and, when require_published != 0,
 *     published[id] != 0 (if no classify has run every flag reads 0): the member test of sdm_vmap_components, word for
 *     word.  The cell of an entry is c = floorf(P_k * inv) of its record point P, as sdm_vmap_components forms it.  A cell
 *     with a coordinate outside [-2^20, 2^20) holds nothing: the range test comes before the key is formed.  Below, "the
 *     member of a cell" is the cell's entry if it exists and is a member.
 *   - Input normal: normal[(id - first)*3 + 0..2] is caller-supplied binary32, normally the output of sdm_vmap_normals over
 *     the same range.  It is only compared, never used in arithmetic.  The axis: a = 0; if (fabsf(n_1) > fabsf(n_a)) a = 1;
 *     if (fabsf(n_2) > fabsf(n_a)) a = 2: ties go to the lower index and a NaN never wins.  Denormals are kept: a denormal
 *     component is > 0.  u = (a+1) mod 3 and v = (a+2) mod 3.
 *   - Owner: entry id of the range is an OWNER iff it is a member, fabsf(n_a) > 0 (false for a NaN, so an all-zero or
 *     NaN-at-a normal owns nothing), and the cell c - e_a holds no member: it is the bottom of its run along a.
 *   - Step: step(j, ax) for ax in {u, v}, in the owner's frame: t = cell(j) + e_ax; for da in the order 0, -1, +1: if the
 *     cell t + da*e_a holds a member k, then at most twice: if the cell below it along -e_a holds a member, take that one
 *     and move down; return the result.  No hit gives NONE.
 *   - Corners: Nu = step(id, u); Nv = step(id, v); C = step(Nu, v) if Nu exists; if C is NONE and Nv exists, C =
 *     step(Nv, u).  The four lie in four distinct columns, so they are distinct ids.
 *   - Triangles of an owner, in this order: all three exist: (id,Nu,C), (id,C,Nv), a QUAD; only Nu and Nv: (id,Nu,Nv);
 *     only Nu and C: (id,Nu,C); only Nv and C: (id,C,Nv), each a SINGLE; otherwise none.  If n_a < 0 the second and third
 *     index of each triangle are swapped: the winding turns towards the normal.
 *   - Outputs: tri, [T][3]: the triangles of the owners in ascending id, an owner's first triangle before its second.
 *     owner_tris[id - first] in {0, 1, 2}.  vertex_used[j], j in [0, M): 1 iff j is a corner of a triangle of this call,
 *     else 0.
 *   - Totals: entries = the size of the range; members and owners are counted within the range; quads; singles;
 *     triangles = 2*quads + singles; vertices = the ones of vertex_used, counted even when that pointer is NULL.
 *   - Range: the entries first .. first + count - 1 (count == -1: to M).  A sub-range returns exactly the whole call's
 *     triangles whose owner lies in it, in order.  An empty range queues nothing and writes no destination.
 *   - Capacity: normal holds 3 x capacity floats and owner_tris capacity bytes, capacity >= the size of the range;
 *     vertex_used holds used_capacity >= M bytes; tri holds 3 x tri_capacity words.  triangles > tri_capacity with tri !=
 *     NULL is SDM_EINVAL; the seven totals are filled and no destination is written (sdm_vmap_classify's and
 *     sdm_vmap_components' contract: counts first, one wait, and the writing launch is queued only if the call is not
 *     refused).  The caller sizes the array and calls again.  The arrays follow args->on_device (there: normal and tri
 *     4-byte aligned).  Any destination may be NULL; all three NULL is valid and returns the totals only.
 *   - State: the call changes nothing in the map or the engine.  Every output is a pure function of the arguments, the
 *     records' cells and multiplicities, and the flags: bitwise the same from run to run, whatever the table layout and the
 *     slicing.
 * Errors, all raised on the host before anything is queued; the seven totals are then 0:
 *   SDM_EINVAL: a NULL ctx or args.
 *   SDM_ESTATE: no open map.
 *   SDM_EINVAL: require_published not 0 or 1; first < 0, count < -1, or first + count > M; a NULL normal with a range that
 *     is not empty; a negative capacity, tri_capacity or used_capacity; capacity below the range; used_capacity < M with
 *     vertex_used given; a misaligned device pointer.
 *   SDM_EHIP: an allocation failure, raised before any launch.
 * Cost: one lane per entry of the range; 12 B of normal, and per owner at most 21 read-only probes (1 + 4 x (3 + 2)), each
 * hit 4 B of multiplicity (+ 1 B of flag); then two passes in tiles for the count and the write, and one over M bytes for
 * the vertices.  Scratch: 13 B per entry of the range and 1 B per entry of the map.  Host normals are staged in, host
 * destinations pass through engine staging: one copy per array of exactly the range (tri: triangles, vertex_used: M)
 * elements.  Two host waits: the totals (56 B), then the end.  Measured: DESIGN.md s.29.
 * Limits: the mesh is voxel-level, at each voxel's winning point; the vertices are the run bottoms only; a missing owner
 * corner loses that cell's triangle; there are seams where the dominant axis changes; the mesh is not watertight; a surface
 * at 45 degrees to two axes (a double tie of the normal's components) is the bad case; the call is O(range) per call, not
 * incremental; the result goes stale with sdm_set_pose as the records do (sdm_vmap_repose re-places them); one rank only. */
typedef struct {
    unsigned min_multiplicity; /* in: as sdm_vmap_components */
    int require_published;     /* in: 0 or 1 */
    int on_device;             /* in: the four arrays are device pointers (normal, tri: 4-byte aligned) */
    long long first, count;    /* in: entries first .. first+count-1; count == -1: to M */
    long long capacity;        /* in: entries normal (x3) and owner_tris hold */
    long long tri_capacity;    /* in: triangles tri holds */
    long long used_capacity;   /* in: bytes vertex_used holds */
    const float *normal;       /* in: [capacity][3] */
    unsigned *tri;             /* [tri_capacity][3] or NULL */
    unsigned char *owner_tris; /* [capacity] or NULL */
    unsigned char *vertex_used;/* [used_capacity] or NULL */
    long long entries, members, owners, quads, singles, triangles, vertices;   /* out */
} sdm_vmap_mesh_args;
int sdm_vmap_mesh(sdm_ctx *ctx, sdm_vmap_mesh_args *args);
/* The most points sdm_extract_points can return for these arguments: the list length of each slot it walks by list,
 * W x H of the others (for sizing buffers without a second call).  Same slot errors; host-blocking only as above. */
int sdm_extract_bound(sdm_ctx *ctx, int n, const int *slots, int source, double min_rho, long long *bound);
/* device addresses for zero-copy interop (RCCL all-gather of per-keyframe {rho,sigma} maps):
 * the depth pool is [max_keyframes][H][W] of float2 {rho,sigma}. */
void *sdm_depth_pool_ptr(sdm_ctx *ctx);
/* The caller asserts that the depth maps of these slots are zero outside the keyframe's active-pixel
 * set {inset pixels with GradImg >= lambdaG} -- true for every map SemiDenseRecon produced, e.g. maps
 * restored through sdm_upload_depth or received by an all-gather.  Lets K2-K4 use their list kernels. */
int sdm_assume_pipeline_maps(sdm_ctx *ctx, int n, const int *slots);

/* Maps written into an ext_depth_pool from outside the engine (the host framework's own collective):
 * marks the slots as holding finished depth maps (kf->semidense_flag_). */
int sdm_mark_depth_present(sdm_ctx *ctx, int n, const int *slots);

/* ---- multi-GPU exchange: the path's one collective step -------------------------- */
/* Keyframes shard in contiguous blocks, one process per GPU.  K1-K3 need no communication; K4
 * (InterKeyFrameDepthChecking, PM.cc:628-799) reads the neighbours' FINISHED {rho,sigma} maps, which
 * cross GPUs once per pass -- over RCCL (xGMI inside a node).  The reference is single-process and has
 * nothing to replace here; SURVEY.md §8(b) sketches this entry as `sdm_allgather`.
 * A communicator is built from an RCCL unique id (rank 0 creates it and hands the 128 bytes to the other
 * ranks through any channel it likes -- a file, MPI, torch.distributed) or borrowed from the caller.
 * With world == 1 every exchange call is a no-op that returns SDM_OK and RCCL is never loaded. */
#define SDM_COMM_ID_BYTES 128
int sdm_comm_unique_id(unsigned char id[SDM_COMM_ID_BYTES]);                 /* ncclGetUniqueId  */
int sdm_comm_init(sdm_ctx *ctx, const unsigned char id[SDM_COMM_ID_BYTES], int world, int rank);
int sdm_comm_attach(sdm_ctx *ctx, void *nccl_comm); /* borrow an existing ncclComm_t (not destroyed) */
int sdm_comm_destroy(sdm_ctx *ctx);
int sdm_comm_info(sdm_ctx *ctx, int *world, int *rank);
/* Halo form: send the maps in send_slot[i] to rank send_peer[i], receive rank recv_peer[i]'s maps into
 * recv_slot[i]; per peer pair the k-th send matches the k-th receive.  _begin returns at once: the
 * transfers run on a second stream behind everything queued so far, and work queued afterwards (the
 * interior keyframes' sdm_recon) overlaps them; sdm_exchange_wait orders later work (sdm_inter_check)
 * behind the transfers.  Neither call waits on the host. */
int sdm_exchange_halo_begin(sdm_ctx *ctx, int n_send, const int *send_peer, const int *send_slot,
                            int n_recv, const int *recv_peer, const int *recv_slot);
int sdm_exchange_wait(sdm_ctx *ctx);
int sdm_exchange_halo(sdm_ctx *ctx, int n_send, const int *send_peer, const int *send_slot,
                      int n_recv, const int *recv_peer, const int *recv_slot); /* begin + wait */
/* All-gather form (BASELINE.json's wording): every rank contributes `count` maps from local slot
 * first_slot on.  n_fetch < 0: in place, the pool holds world*count slots with slot == global
 * keyframe index and first_slot == rank*count.  n_fetch >= 0: gathered into an engine-owned buffer;
 * map number fetch_index[i] (= owner_rank*count + position in the owner's block) is copied into local
 * slot dst_slot[i].  Stream-ordered; no host wait. */
int sdm_allgather_depth(sdm_ctx *ctx, int first_slot, int count, int n_fetch, const int *fetch_index,
                        const int *dst_slot);
/* The all-gather in pieces, overlapped with the reconstruction.  Every rank contributes maps_per_rank maps (the
 * same number on all ranks) in one or more pieces: _piece(count, slots) -- count equal on all ranks, padded by
 * repeating a slot if a rank has fewer -- is called right after the sdm_recon of those keyframes and gathers them on a
 * second stream behind an event, so the next sdm_recon overlaps the transfer; _finish orders later work
 * (sdm_inter_check) behind the last piece and copies the maps this rank reads (fetch_index = owner_rank *
 * maps_per_rank + position in the owner's contribution order) into dst_slot.  Used for the whole block in sub-blocks,
 * or for just the keyframes other ranks read (a third of the bytes on an index-local covisibility graph).
 * The fetch copies run on the second stream too: between _begin and _finish the caller must not queue work that
 * reads or writes the depth maps of the dst_slot keyframes -- anything else (sdm_recon of the next keyframes,
 * sdm_inter_check of keyframes whose neighbours are all local) overlaps the transfer AND the copies.
 * No host wait.  world == 1: the pieces are device copies and the fetch addressing still runs. */
int sdm_allgather_begin(sdm_ctx *ctx, int maps_per_rank);
int sdm_allgather_piece(sdm_ctx *ctx, int count, const int *slots);
int sdm_allgather_finish(sdm_ctx *ctx, int n_fetch, const int *fetch_index, const int *dst_slot);
/* Wire format of the maps that cross ranks in sdm_exchange_halo[_begin] and sdm_allgather_piece / _finish.
 * entries_per_map = 0 (default): whole maps, 8*W*H bytes each.  > 0: the {rho,sigma} of the first entries_per_map entries
 * of the keyframe's active-pixel list (the pixels that pass the gradient gate, PM.cc:201), in list order -- all a
 * reconstructed map holds, since it is zero elsewhere: 8*entries_per_map bytes (a fifth of the map on typical images).
 * The receiver scatters them through ITS list of that keyframe, which it has because the keyframe is part of its input
 * halo (SDM_ESTATE if the destination slot holds no keyframe).  Every rank must set the same value, at least the longest
 * list (sdm_active_count) among the keyframes it sends or receives; a call that meets a longer one fails with SDM_ESTATE
 * before posting anything -- so agree on the value across ranks beforehand (bench.py: an all-reduce(max) at set-up).
 * sdm_allgather_depth (the one-shot form) always moves whole maps and refuses to run while entries_per_map > 0.
 * sdm_comm_destroy resets the format to whole maps. */
int sdm_exchange_compact(sdm_ctx *ctx, int entries_per_map);
/* Every compact map carries its sender's list length and the 64-bit hash of its list; a receiver whose list of that
 * keyframe differs in either (its image differs from the sender's) does not scatter the map -- it would land on wrong
 * pixels -- and counts the event: a destination that already held a pipeline map keeps it; one that did not (an arbitrary
 * map, e.g. from sdm_upload_depth) has been zeroed for the scatter and stays zero.  *count = such maps since the last call
 * (host-blocking; 0 on a healthy job). */
int sdm_exchange_mismatches(sdm_ctx *ctx, int *count);
/* The compact wire format through host memory, one map per call (host-blocking): the payload the RCCL forms would send
 * for `slot` -> out[2 * (entries_per_map + 8)] floats ({rho,sigma} of the list entries, then the header: list length
 * and hash), and the receiving side for a payload that travelled by another route (*refused = 1: packed with another
 * list; checked on the host before anything is written: the slot's plane is left alone).  Same kernels and checks as sdm_exchange_* -- for transports the engine does not
 * drive (a host framework's own, or gloo on a one-GPU box: shard.py). */
int sdm_compact_pack_host(sdm_ctx *ctx, int slot, float *out);
int sdm_compact_unpack_host(sdm_ctx *ctx, int slot, const float *in, int *refused);
/* *ready = 1 iff every listed slot's map would be accepted as a compact SOURCE now (a pipeline map under the current
 * lambdaG); the query form of the check the compact sends make.  Fold it into the per-pass wire-format agreement
 * (ProbabilityMapping::SemiDenseReconBlock does): a rank that answers 0 makes all ranks use whole maps for the pass. */
int sdm_compact_sources_ready(sdm_ctx *ctx, int n, const int *slots, int *ready);
/* Length of the slot's active-pixel list under the current lambdaG (built now if need be; host-blocking). */
int sdm_active_count(sdm_ctx *ctx, int slot, int *count);
/* The list itself, (y << 16 | x) of the inset pixels with GradImg >= lambdaG in raster order (PM.cc:198-201), and the
 * 64-bit hash of that pixel set the compact wire header carries; any output may be NULL.  For tests and for rehearsing
 * the compact exchange on host arrays (orb-slam-free-space-carving_amd/shard.py). */
int sdm_download_active_list(sdm_ctx *ctx, int slot, unsigned *list, int capacity, int *count,
                             unsigned long long *hash);
/* Go / no-go before a collective pass: all ranks call it; *all_ok = min over ranks of local_ok (host-blocking).
 * A rank that cannot take part in the exchange it planned reports it here, so peers skip the pass instead of
 * waiting for transfers that never come. */
int sdm_comm_all_ok(sdm_ctx *ctx, int local_ok, int *all_ok);
/* *all_max = max over ranks of local_value (all ranks call it; host-blocking; world size 1: the local value) -- e.g. the
 * longest active list of the job, for sdm_exchange_compact. */
int sdm_comm_all_max(sdm_ctx *ctx, int local_value, int *all_max);

/* ---- stand-alone map operations with the reference's signatures -------------------------------- */
/* IntraKeyFrameDepthChecking(cv::Mat&, cv::Mat&, const cv::Mat) PM.h:85; host maps, in place. */
int sdm_intra_check_maps(sdm_ctx *ctx, float *rho, float *sigma, const float *grad);
/* IntraKeyFrameDepthGrowing(cv::Mat&, cv::Mat&, const cv::Mat)  PM.h:86 */
int sdm_intra_grow_maps(sdm_ctx *ctx, float *rho, float *sigma, const float *grad);

/* ---- per-pixel entry points (unit tests; same device functions as the batched kernels) -------- */
/* EpipolarSearch PM.h:79: out = {rho, sigma, supported(0/1), best_u, best_v} */
int sdm_epipolar_search(sdm_ctx *ctx, int ref_slot, int nbr_slot, int x, int y, float min_depth,
                        float max_depth, float rot_deg, float out[5]);
/* GetSearchRange PM.h:80 */
int sdm_search_range(sdm_ctx *ctx, int ref_slot, int nbr_slot, int x, int y, float mind,
                     float maxd, float *umin, float *umax);
/* InverseDepthHypothesisFusion PM.h:83: out = {rho, sigma, supported(0/1)} */
int sdm_fuse(sdm_ctx *ctx, const float *rho, const float *sigma, int n, float out[3]);
/* ComputeFundamental PM.h:101 and R21/t21 (PM.cc:859-860): F12[9], R21[9], t21[3] */
int sdm_pair_geometry(sdm_ctx *ctx, int ref_slot, int nbr_slot, float F12[9], float R21[9],
                      float t21[3]);

/* ---- host helpers of the class surface (no device work) ---------------------------------------- */
/* StereoSearchConstraints PM.h:77 / PM.cc:370-383 over the keyframe's ORB point depths */
int sdm_stereo_search_constraints(const float *orb_depths, int n, float *min_depth,
                                  float *max_depth);
/* GetRotInPlane PM.h:103 / PM.cc:467-484 + the median of PM.cc:170-179; ids < 0 = no map point */
float sdm_median_rot_in_plane(const int *mp1, const float *angle1, int n1, const int *mp2,
                              const float *angle2, int n2);

/* ---- instrumentation ---------------------------------------------------------------------------- */
/* when enabled, sdm_search_fuse runs its counting variant (slower) and accumulates into stats */
int sdm_enable_stats(sdm_ctx *ctx, int on);
int sdm_get_stats(sdm_ctx *ctx, sdm_stats *out, int reset);
/* diagnostic: how sdm_search_fuse / sdm_recon / sdm_epipolar_search walk the candidate range of PM.cc:405 -- 0 (default): per
 * wave and neighbour, from the wave's range lengths and line slopes; 1: always the batched scan; 2: always the scan over the
 * neighbour's gradient-gate bit plane.  Results are the same bit for bit in every mode (tests/test_gpu_longscan.py). */
int sdm_set_scan_mode(sdm_ctx *ctx, int mode);
/* Every launch whose grid grows with data goes out in groups of dispatches of at most 2^31 work-items (a test lowers the limit
 * per context: SDM_MAX_DISPATCH_LOG2 in [8, 31], read by sdm_create).  What this context issued since the last reset, counted
 * on the host (nothing is read from the device, nothing waits; sdm_stats does not move): out[0] = groups, out[1] = dispatches,
 * out[2] = groups that took more than one dispatch.  With the default limit out[2] stays 0 below 2^31 work-items per launch. */
int sdm_get_dispatch_counts(sdm_ctx *ctx, long long out[3], int reset);
/* Streaming ingest (default off).  On: the batched uploads (sdm_upload_images_batch / _rgb_batch) get twelve chunk buffers
 * instead of four, so the host staging and the H2D copies (upload stream) of up to three 64-keyframe blocks run ahead of
 * their pre-pass kernels, which stay on the compute stream in call order (and, the copies being ahead anyway, run as ONE
 * launch per group of four chunks behind one wait for the group's last copy).  A block uploaded BEFORE the previous block's step
 * is queued (double-buffer the slot sets: bench.py streaming_rate; frames arrive continuously in the fork,
 * src/Tracking.cc:266-271) is then copied while that step runs, pre-processed right behind it, and its list lengths are back
 * before its own step is queued (every compute call waits for the list lengths of ITS slots only, with or without this
 * switch).  Results are the serial order's by construction (one compute stream).  Costs 8 x the chunk size of device and
 * pinned host memory (8 x 4.9 MB at 640x480).  Host-blocking when it allocates. */
int sdm_set_ingest_overlap(sdm_ctx *ctx, int on);
/* per-stage device time measured with HIP events recorded on the context's stream around each
 * stage's kernel launches (K1 = one k_search_fuse launch per sdm_recon/sdm_search_fuse call) */
#define SDM_STAGE_SEARCH_FUSE 0 /* K1   PM.cc:197-231 */
#define SDM_STAGE_INTRA 1       /* K2+K3 PM.cc:237-238 */
#define SDM_STAGE_INTER 2       /* K4   PM.cc:628-799 */
#define SDM_STAGE_POINTSET 3    /* K5   PM.cc:337-367 */
#define SDM_NUM_STAGES 4
int sdm_enable_timing(sdm_ctx *ctx, int on);
int sdm_get_timing(sdm_ctx *ctx, double ms_total[SDM_NUM_STAGES], long long launches[SDM_NUM_STAGES],
                   int reset);
/* device arithmetic self-tests: out[0] = mismatches (must be 0), out[1] = auxiliary count.
 * which 0: reciprocal+FMA division by theta_var vs plain division over all 2^32 float inputs;
 * which 1: reciprocal-prefiltered ChiTest vs the exact ChiTest around the 5.99 threshold;
 * which 2: fast matching cost (PM.cc:436) vs the reference expression incl. rounding midpoints, and the distance of
 *          the scan's approximate cost from it (at most 4 float steps: the arg-min of PM.cc:437 compares exactly);
 * which 3: closed-form angle gates (PM.cc:414-431) vs the reference statement;
 * which 4: GetFusion's shared-reciprocal double quotients (PM.cc:956-957) vs plain divisions;
 * which 5: reciprocal-form float quotients (K4, PM.cc:678-680,782-783; the line quotients PM.cc:393,407) vs IEEE
 *          divisions inside the operand windows, all-ones divisor significands included;
 * which 6: reciprocal + one FMA step (K4/K5, PM.cc:769,777,793,349) vs IEEE 1/b, and rsq + one FMA step (PM.cc:818)
 *          vs sqrtf, over all 2^32 float inputs;
 * which 7: K4's straight-line per-neighbour body vs the reference statement (PM.cc:677-755,777-783) on 5*10^8
 *          random geometries / 2x2 tap patches; out[1] = cases whose fast result was accepted;
 * which 8: scan identities (lerp weight, in-plane-rotation wrap) over all 2^32 float inputs;
 * which 9: the same run as 7, reporting out[1] = projections (PM.cc:677-680, 695) decided by K4's approximate chain --
 *          each compared with the plain-division chain's cell, validity and offset;
 * which 10: K1's fast_atan2_deg_x1 (PM.cc:414) vs fast_atan2_deg(y, 1) over all 2^32 float inputs; out[1] = an
 *          order-independent 64-bit digest of its results, equal to OpenCV 2.4.5's cvFastArctan(y, 1)
 *          (tests/golden/fastatan2_x1_digest.json);
 * which 11: the reciprocal-form quotient vs the IEEE division over the operand ranges K1's per-pair boxes prove (range,
 *          sigma and Eq. 8 quotients, PM.cc:896-897, 457, 845-875): divisors in [2^-30, 2^30], numerators +0 or in
 *          [2^-66, 2^40], both signs, all-ones significands; out[1] = 2^32 pairs;
 * which 12: no arithmetic -- out[0] = pairs of the last compute call whose search-range quotients take the reciprocal
 *          form, + (pairs whose sigma / Eq. 8 quotients do) << 32; out[1] = pairs of that call;
 * which 13, 14, 15: K1's decided f64 roundings vs the statements as written -- 13 ustar (PM.cc:458), 14 GetFusion's two
 *          sums over chains of 1..20 terms (PM.cc:936-937), 15 GetFusion's pjsj / rsj and sqrtf(1 / rsj) (PM.cc:225-226);
 *          out[1] = draws inside the operand window that were handed to the statement (undecided), out of
 *          2^27 (13), 330301440 (14) and 2^28 (15) such draws; draws outside the windows and special operands on top;
 * which 16, 17, 18: no arithmetic -- where the keys of a hash table sit, for tests that force long probes: out[0] = the
 *          largest (slot - home) & mask over the occupied slots, home = the key's hash & mask; out[1] = occupied slots with
 *          slot < home, i.e. keys whose probe went past the end of the table.  16 the voxel map's table, 17 its observation
 *          set (0, 0 before the first observation), both SDM_ESTATE without an open map; 18 the per-call table the last
 *          sdm_extract_points_voxel* call with a plain point left in the context's scratch (SDM_ESTATE: none).  Read-only:
 *          nothing any other call returns depends on them. */
int sdm_selftest(sdm_ctx *ctx, int which, unsigned long long out[2]);
/* name of the device the context runs on, e.g. "gfx950" */
const char *sdm_device_arch(sdm_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
