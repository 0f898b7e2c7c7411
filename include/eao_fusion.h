/* eao_fusion.h -- C-ABI of libeaofusion_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for EAO-Fusion's ORB front-end + local-BA hot path.  The reference has no FFI/plugin
 * layer: its boundary is the C++ class surface ORB_SLAM2::{ORBextractor, ORBmatcher, Optimizer}.  The
 * header-only adapters in include/eaofusion/ keep those signatures and call the functions below; every
 * entry point cites the reference interface it stands behind.  Plain pointers and sizes only -- no C++,
 * OpenCV, Eigen or torch types cross this ABI.
 *
 * Conventions
 *  - every function returns eao_status (0 = ok, < 0 = error) and never throws; eao_last_error() gives the
 *    thread-local message of the last failure.
 *  - the caller allocates all outputs; the library owns device memory inside handles.
 *  - "_device" variants take pointers that are already resident in HBM and a hipStream_t passed as void*
 *    (NULL = the null stream); they enqueue work on that stream and do NOT synchronise.
 *  - a handle is single-threaded (one HIP stream each); distinct handles are independent; the stateless
 *    functions are thread-safe.
 *  - there is NO CPU fallback: without a usable HIP device every compute entry point fails with
 *    EAO_ERR_NO_DEVICE.
 */
#ifndef EAO_FUSION_H_
#define EAO_FUSION_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t eao_status;
enum {
    EAO_OK = 0,
    EAO_ERR_INVALID = -1,    /* bad argument / unsupported geometry */
    EAO_ERR_NO_DEVICE = -2,  /* no HIP device or HIP runtime failure */
    EAO_ERR_CAPACITY = -3,   /* caller-provided output capacity too small */
    EAO_ERR_INTERNAL = -4
};

const char* eao_last_error(void);
/* 0 when a gfx950-class device is usable by this process, else EAO_ERR_NO_DEVICE (never initialises a context
 * beyond hipGetDeviceCount / hipGetDeviceProperties). */
eao_status eao_device_check(void);
const char* eao_version(void);

/* ------------------------------------------------------------------------------------------------
 * ORB extraction -- replaces ORB_SLAM2::ORBextractor
 *   ctor        reference include/ORBextractor.h:52-53, src/ORBextractor.cc:410-470
 *   operator()  reference include/ORBextractor.h:60-62, src/ORBextractor.cc:1043-1105
 * ------------------------------------------------------------------------------------------------ */
typedef struct eao_orb eao_orb; /* opaque handle */

typedef struct {
    int32_t nfeatures;   /* ORBextractor.nFeatures  */
    float scale_factor;  /* ORBextractor.scaleFactor */
    int32_t nlevels;     /* ORBextractor.nLevels (1..16) */
    int32_t ini_th_fast; /* ORBextractor.iniThFAST */
    int32_t min_th_fast; /* ORBextractor.minThFAST */
} eao_orb_cfg;

/* cv::KeyPoint POD mirror (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} eao_keypoint;

eao_status eao_orb_create(const eao_orb_cfg* cfg, eao_orb** out);
void eao_orb_destroy(eao_orb* h);

/* scale tables exposed by the reference getters (include/ORBextractor.h:63-83); arrays of nlevels floats/ints,
 * any pointer may be NULL */
eao_status eao_orb_tables(const eao_orb* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                          int32_t* features_per_level);

/* Upper bound on keypoints returned per frame of the given size (the quad-tree can return a few more than
 * nfeatures: it stops at the first list size >= quota).  Use it to size kps/desc. */
eao_status eao_orb_max_keypoints(eao_orb* h, int32_t width, int32_t height, int32_t* cap);

/* One frame from host memory, synchronous: operator()(image, mask, keypoints, descriptors).
 * img: 8-bit single channel, `stride` bytes per row.  kps/desc: capacity `cap` keypoints (desc = cap*32 bytes).
 * *n receives the number of keypoints.  Empty image (img NULL or w/h <= 0) => *n = 0, outputs untouched
 * (reference src/ORBextractor.cc:1046-1047). */
eao_status eao_orb_extract(eao_orb* h, const uint8_t* img, int32_t width, int32_t height, int32_t stride,
                           eao_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n);

/* Batch of `batch` same-sized frames from host memory, synchronous.  Frame f starts at img + f*frame_stride.
 * kps: batch*cap entries, desc: batch*cap*32 bytes, n: batch counts. */
eao_status eao_orb_extract_batch(eao_orb* h, const uint8_t* img, int32_t width, int32_t height, int32_t stride,
                                 int64_t frame_stride, int32_t batch, eao_keypoint* kps, uint8_t* desc, int32_t cap,
                                 int32_t* n);

/* Streaming host API: what feeds Frame::ExtractORB are HOST images (reference src/Frame.cc:616-622, behind the Frame constructors
 * :192-194), and a sequence reader has the next batch ready while this one is extracted.  The handle owns `nslots` slots of PINNED
 * host memory: the producer writes up to `batch` frames into eao_orb_slot.frames (rows of `stride` bytes, frames `frame_stride`
 * apart), eao_orb_stream_submit is ASYNCHRONOUS (upload -> extraction -> download on three streams, chained by events: the upload
 * of one slot and the download of another overlap the extraction of a third), eao_orb_stream_wait blocks until the slot's results
 * are in its pinned kps / desc / n arrays (frame f: kps + f * cap, desc + f * cap * 32, n[f]).  Results are those of
 * eao_orb_extract_batch on the same frames.  A slot may be refilled once it has been waited for; submit on a slot that is still in
 * flight waits for it first.  One producer thread per handle. */
typedef struct {
    uint8_t* frames;          /* pinned: batch x height rows of `stride` bytes */
    int32_t stride;           /* row pitch of `frames` (>= width, a multiple of 64) */
    int64_t frame_stride;     /* stride * height */
    eao_keypoint* kps;        /* pinned: batch x cap */
    uint8_t* desc;            /* pinned: batch x cap x 32 */
    int32_t* n;               /* pinned: batch */
    int32_t cap;              /* = eao_orb_max_keypoints */
} eao_orb_slot;
eao_status eao_orb_stream_create(eao_orb* h, int32_t width, int32_t height, int32_t batch, int32_t nslots);
eao_status eao_orb_stream_slot(eao_orb* h, int32_t slot, eao_orb_slot* out);
eao_status eao_orb_stream_submit(eao_orb* h, int32_t slot, int32_t batch);
eao_status eao_orb_stream_wait(eao_orb* h, int32_t slot);

/* Same, all pointers device-resident (HBM), asynchronous on `stream` (a hipStream_t; NULL = the null stream, exactly as the
 * Hamming entry points read it): whatever the caller enqueues on that stream afterwards is ordered behind the extraction.
 * The main chain of the call's kernels is enqueued on `stream` ITSELF (a private side stream of the handle, forked from and
 * joined back into it with events, carries the part that runs beside it), so consecutive calls on one stream follow each
 * other without a cross-stream hop.  Calls on one handle are serialised with each other even when they come in on different
 * streams (they share the handle's pyramid and candidate scratch): a call on another stream than the previous one first drains
 * the device on the host (hipDeviceSynchronize -- the previous stream's handle is never used again, so its owner is free to
 * destroy it once its own work is done).  NULL is the legacy null stream (rounds 1 - 2a read NULL as "the handle's private
 * stream"; callers that relied on that pass their own stream now).  d_n: batch int32 on the device. */
eao_status eao_orb_extract_batch_device(eao_orb* h, const uint8_t* d_img, int32_t width, int32_t height,
                                        int32_t stride, int64_t frame_stride, int32_t batch, eao_keypoint* d_kps,
                                        uint8_t* d_desc, int32_t cap, int32_t* d_n, void* stream);

/* Pyramid level of frame `frame` of the LAST extract call, copied to host (tight rows, w*h bytes): backs the
 * public member ORBextractor::mvImagePyramid (include/ORBextractor.h:85).  which = 0 level image, 1 = its
 * 7x7 Gaussian-blurred copy.  Either of w/h/dst may be NULL to query sizes only. */
eao_status eao_orb_level(eao_orb* h, int32_t frame, int32_t level, int32_t which, int32_t* w, int32_t* hgt, uint8_t* dst);

/* ALL levels of frame `frame` of the last extraction in ONE call, each with a `border`-pixel BORDER_REFLECT_101 frame physically around it -- the form
 * upstream keeps in mvImagePyramid (EDGE_THRESHOLD = 19: src/ORBextractor.cc:1113-1128; read by Frame::ComputeStereoMatches only, src/Frame.cc:846, 936-953).
 * One launch writes the bordered levels into a pinned host block the handle owns; levels[l] (nlevels entries) receives the address of the level's pixel
 * (0, 0) inside it, its size and its row pitch (rows -border .. height + border - 1 and columns -border .. width + border - 1 are addressable around it).
 * The block is valid until the next eao_orb_pyramid call on the handle or its destruction.  After a host-API extraction (eao_orb_extract*) nothing but the
 * handle's own stream is synchronised; after eao_orb_extract_batch_device on a caller's stream the device is drained first. */
typedef struct {
    uint8_t* data;            /* pixel (0, 0) of the level */
    int32_t width, height;
    int32_t step;             /* bytes per row */
} eao_orb_level_view;
eao_status eao_orb_pyramid(eao_orb* h, int32_t frame, int32_t border, eao_orb_level_view* levels);
/* border >= 0: every eao_orb_extract_ref call also exports the frame's bordered pyramid behind the extraction, on the same stream and under the same single
 * synchronisation, and the eao_orb_pyramid call that follows only hands out the views; -1 (the default): off. */
eao_status eao_orb_set_keep_pyramid(eao_orb* h, int32_t border);

/* eao_orb_extract without the copy into caller arrays: *kps / *desc point into the pinned block the device wrote the frame's results to (*n keypoints,
 * *n x 32 descriptor bytes), valid until the next call on the handle.  What the class-surface adapter uses: its cv::KeyPoint vector and descriptor matrix
 * are filled straight from there. */
eao_status eao_orb_extract_ref(eao_orb* h, const uint8_t* img, int32_t width, int32_t height, int32_t stride, const eao_keypoint** kps,
                               const uint8_t** desc, int32_t* n);

/* Stage taps for parity tests (device -> host copies of intermediate products of the LAST extract call).
 * candidates: FAST corners of (frame, level) in reference order before the quad-tree, as (x, y, response)
 * float triples relative to the (16,16) level border origin; returns the count in *n (cap in triples). */
eao_status eao_orb_level_candidates(eao_orb* h, int32_t frame, int32_t level, float* xyr, int32_t cap, int32_t* n);

/* HIP-event timing of the pipeline stages, in milliseconds, in pipeline order:
 * [0] pyramid  [1] fast  [2] quadtree  [3] blur  [4] orient+describe  [5] whole pipeline,
 * AVERAGED over every extract call made since eao_orb_set_profiling(h, 1) (events are recorded on the stream the
 * kernels run on); reading blocks until the events have completed and restarts the average.  The blur runs on a side
 * stream concurrently with FAST + quad-tree, so the stage times may add up to more than [5].
 * eao_orb_lanes() returns the number of concurrent slices a batch is cut into: always 1 (one pipeline per call). */
eao_status eao_orb_set_profiling(eao_orb* h, int32_t on);
eao_status eao_orb_last_timing(eao_orb* h, float ms[6]);
int32_t eao_orb_lanes(int32_t batch);

/* ------------------------------------------------------------------------------------------------
 * Hamming matching -- replaces ORBmatcher::DescriptorDistance (reference src/ORBmatcher.cc:1649-1665) and
 * the candidate loops of the Search* routines (e.g. :83-115, :1402-1426)
 * ------------------------------------------------------------------------------------------------ */
/* D[i*nb + j] = popcount(A_i xor B_j), A: na x 32 bytes, B: nb x 32 bytes (host pointers, synchronous) */
eao_status eao_hamming_matrix(const uint8_t* A, int32_t na, const uint8_t* B, int32_t nb, uint16_t* D);

typedef struct {
    int32_t best;    /* smallest distance, 256 if no candidate */
    int32_t second;  /* second smallest (reference bestDist2), 256 if none */
    int32_t idx;     /* column of best, -1 if none; first column wins ties (strict '<' upstream) */
    int32_t idx2;    /* column of second, -1 if none */
} eao_best2;
/* per row of A the best two over the columns j with mask[i*nb + j] != 0 (mask NULL = all) */
eao_status eao_hamming_best2(const uint8_t* A, int32_t na, const uint8_t* B, int32_t nb, const uint8_t* mask,
                             eao_best2* out);

/* device-resident variants; `pairs` independent (A,B) problems laid out back to back (pair p: A + p*na*32, ...) */
eao_status eao_hamming_matrix_device(const uint8_t* d_A, int32_t na, const uint8_t* d_B, int32_t nb, int32_t pairs,
                                     uint16_t* d_D, void* stream);
eao_status eao_hamming_best2_device(const uint8_t* d_A, int32_t na, const uint8_t* d_B, int32_t nb, int32_t pairs,
                                    const uint8_t* d_mask, eao_best2* d_out, void* stream);

/* The consecutive-frame matcher of a device-resident batch (BASELINE configs[4]): pair f = (frame f - 1,
 * frame f) for every frame of the descriptor block d_desc [batch][cap][32] an eao_orb_extract_batch_device call left on
 * the device, with the per-frame keypoint counts read ON THE DEVICE from d_counts (that call's d_n) -- no host round trip
 * between extraction and matching.  Result of pair f, row i < count[f - 1]: d_out[f * cap + i] = the two nearest
 * descriptors of frame f (same definition as eao_hamming_best2).  Pair 0 matches the halo frame (d_halo_desc, halo_n rows:
 * the last frame of the previous shard) against frame 0, or is skipped when halo_n == 0.  Rows beyond a pair's count are
 * not written. */
eao_status eao_hamming_best2_sequence_device(const uint8_t* d_desc, int32_t cap, const int32_t* d_counts, int32_t batch,
                                             const uint8_t* d_halo_desc, int32_t halo_n, eao_best2* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Guided matching -- ORBmatcher::SearchByProjection, the two per-frame tracking variants
 *   (Frame&, const vector<MapPoint*>&, th)          reference src/ORBmatcher.cc:45-129   (TrackLocalMap)
 *   (Frame& Cur, const Frame& Last, th, bMono)      reference src/ORBmatcher.cc:1328-1472 (TrackWithMotionModel)
 * with Frame::GetFeaturesInArea / PosInGrid (src/Frame.cc:696-761) as the candidate generator.  The device builds,
 * for every query, the candidate list (keypoint index, Hamming distance) in the reference's candidate ORDER (grid cell
 * column-major, then insertion order) with every geometric / level / stereo gate applied; the greedy assignment
 * ("skip keypoints that already hold a map point", best / second-best, ratio test, rotation histogram) is replayed
 * on the host inside the library, query by query, exactly as upstream's loops run.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n;                   /* Frame::N */
    const float* kp_x;           /* mvKeysUn[i].pt.x */
    const float* kp_y;
    const int32_t* kp_octave;    /* mvKeysUn[i].octave */
    const float* kp_angle;       /* mvKeysUn[i].angle (rotation histogram) */
    const float* u_right;        /* mvuRight[i] */
    const uint8_t* descriptors;  /* mDescriptors: n x 32 */
    const uint8_t* occupied;     /* n: mvpMapPoints[i] != NULL && Observations() > 0 on entry (may be NULL = none) */
    float min_x, min_y, max_x, max_y;   /* mnMinX, mnMinY, mnMaxX, mnMaxY */
    float grid_inv_w, grid_inv_h;       /* mfGridElementWidthInv, mfGridElementHeightInv */
    int32_t grid_cols, grid_rows;       /* FRAME_GRID_COLS, FRAME_GRID_ROWS (64 x 48 upstream) */
    const float* scale_factors;         /* mvScaleFactors */
    int32_t nlevels;
    /* only read by the entry points that say so (may be 0 / NULL otherwise) */
    float log_scale_factor;             /* mfLogScaleFactor */
    const float* level_sigma2;          /* mvLevelSigma2 */
    const float* inv_level_sigma2;      /* mvInvLevelSigma2 */
} eao_frame_view;

/* SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th): map points that are in view.
 * Per map point: mTrackProjX/Y/XR, mTrackViewCos, mnTrackScaleLevel, GetDescriptor(), and skip[i] != 0 where upstream
 * `continue`s (!mbTrackInView || isBad()).  match_kp[i] receives the keypoint index the point was assigned to or -1;
 * the return value of the reference is *nmatches.  A keypoint assigned during the call counts as occupied afterwards
 * (upstream: F.mvpMapPoints[idx]->Observations() > 0 for a point of the local map). */
eao_status eao_search_by_projection_points(const eao_frame_view* F, int32_t n_mp, const float* proj_x, const float* proj_y,
                                           const float* proj_xr, const float* view_cos, const int32_t* pred_level,
                                           const uint8_t* mp_desc, const uint8_t* skip, float th, float nnratio,
                                           int32_t* match_kp, int32_t* nmatches);

/* SearchByProjection(Frame& Cur, const Frame& Last, th, bMono).  Per last-frame keypoint i: valid[i] != 0 where
 * LastFrame.mvpMapPoints[i] != NULL && !mvbOutlier[i]; Xw = GetWorldPos(); mp_desc = GetDescriptor(); last_octave =
 * LastFrame.mvKeys[i].octave; last_angle = LastFrame.mvKeysUn[i].angle.  Tcw_cur / Tcw_last: 16 floats row-major.
 * cur_match[k] (Cur->n entries) receives the last-frame index assigned to current keypoint k or -1 (after the rotation
 * consistency filter when check_orientation != 0). */
eao_status eao_search_by_projection_frames(const eao_frame_view* Cur, const float* Tcw_cur, const float* Tcw_last,
                                           int32_t n_last, const uint8_t* valid, const float* Xw, const uint8_t* mp_desc,
                                           const int32_t* last_octave, const float* last_angle, float fx, float fy, float cx,
                                           float cy, float mbf, float mb, float th, int32_t mono, int32_t check_orientation,
                                           int32_t* cur_match, int32_t* nmatches);

/* Map points as plain arrays (what the remaining searches read through MapPoint's accessors). */
typedef struct {
    int32_t n;
    const uint8_t* active;        /* n: 0 where upstream `continue`s before looking at the point (NULL pointer, isBad(),
                                     member of the caller's "already found" set, IsInKeyFrame(pKF), ...) */
    const float* Xw;              /* n*3  GetWorldPos() */
    const float* normal;          /* n*3  GetNormal()  (NULL for the searches that have no viewing-angle test) */
    const float* min_dist_inv;    /* n    GetMinDistanceInvariance() */
    const float* max_dist_inv;    /* n    GetMaxDistanceInvariance() */
    const float* max_dist;        /* n    mfMaxDistance, the numerator of PredictScale (src/MapPoint.cc:385-394) */
    const uint8_t* desc;          /* n*32 GetDescriptor() */
} eao_map_points;

/* DBoW2::FeatureVector of one frame: nodes in ascending id, each with its keypoint indices (std::map order). */
typedef struct {
    int32_t n_nodes;
    const uint32_t* node_id;      /* n_nodes, strictly ascending */
    const int32_t* node_start;    /* n_nodes + 1 offsets into index */
    const uint32_t* index;        /* keypoint indices, in the order of the node's vector */
} eao_feature_vector;

/* a13  SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th)
 * -- src/ORBmatcher.cc:290-403 (loop detection).  KF->occupied[k] != 0 where vpMatched[k] != NULL on entry; active[i] = 0
 * for bad points and members of spAlreadyFound.  Reads KF->log_scale_factor.  kp_match[k] receives the index of the point
 * assigned to keypoint k during the call, or -1. */
eao_status eao_search_by_projection_sim3(const eao_frame_view* KF, const float* Scw, float fx, float fy, float cx, float cy,
                                         const eao_map_points* pts, int32_t th, int32_t* kp_match, int32_t* nmatches);

/* a13  SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * -- src/ORBmatcher.cc:1474-1601 (relocalisation).  pts = pKF->GetMapPointMatches() (active[i] = 0 for NULL, bad or already
 * found), kf_angle[i] = pKF->mvKeysUn[i].angle; Cur->occupied = CurrentFrame.mvpMapPoints[k] != NULL.  cur_match[k]
 * receives the map-point index assigned to current keypoint k or -1 (after the rotation filter, whose histogram factor
 * is 1/HISTO_LENGTH here, :1486). */
eao_status eao_search_by_projection_kf(const eao_frame_view* Cur, const float* Tcw, float fx, float fy, float cx, float cy,
                                       const eao_map_points* pts, const float* kf_angle, float th, int32_t orb_dist,
                                       int32_t check_orientation, int32_t* cur_match, int32_t* nmatches);

/* a14  SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) -- src/ORBmatcher.cc:159-288 (mode 0) and
 *      SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) -- :522-655 (mode 1).
 * Side 1 is the keyframe whose map points drive the search: valid1[i] != 0 where its map point exists and is not bad.
 * mode 0: side 2 is the frame; a frame keypoint taken during the call is skipped afterwards; accept best <= TH_LOW.
 * mode 1: valid2[j] != 0 where pKF2's map point exists and is not bad; accept best < TH_LOW.
 * Both: best < nnratio * second.  match12[i] receives the side-2 index matched to side-1 keypoint i or -1. */
eao_status eao_search_by_bow(int32_t mode, int32_t n1, const uint8_t* desc1, const float* angle1, const uint8_t* valid1,
                             const eao_feature_vector* fv1, int32_t n2, const uint8_t* desc2, const float* angle2,
                             const uint8_t* valid2, const eao_feature_vector* fv2, float nnratio, int32_t check_orientation,
                             int32_t* match12, int32_t* nmatches);

/* a15  SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) -- src/ORBmatcher.cc:657-823, with
 * CheckDistEpipolarLine :140-157.  K1 / K2: keypoints (kp_x, kp_y, kp_octave, kp_angle, u_right, descriptors;
 * occupied[k] != 0 where the keyframe already has a map point at k); K2->level_sigma2 and K2->scale_factors are read.
 * F12: 9 floats row-major; (ex, ey) the epipole in image 2 (:663-670).  match12[i] = index in K2 or -1. */
eao_status eao_search_for_triangulation(const eao_frame_view* K1, const eao_feature_vector* fv1, const eao_frame_view* K2,
                                        const eao_feature_vector* fv2, const float* F12, float ex, float ey,
                                        int32_t only_stereo, int32_t check_orientation, int32_t* match12, int32_t* nmatches);

/* The same for ALL neighbour keyframes of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:211-290 calls SearchForTriangulation once per neighbour,
 * 10 or 20 per new keyframe) in one call: one upload of K1 and of every neighbour, one launch, one copy back.  K2s / fv2s: n_nb pointers; F12s: 9 floats
 * per neighbour; exs / eys: the epipoles; match12: n_nb x K1->n (row k = the single call's match12 against neighbour k), nmatches: n_nb.  Equal to n_nb
 * single calls, entry for entry (tests/test_gpu_search.py). */
eao_status eao_search_for_triangulation_batch(const eao_frame_view* K1, const eao_feature_vector* fv1, int32_t n_nb, const eao_frame_view* const* K2s,
                                              const eao_feature_vector* const* fv2s, const float* F12s, const float* exs, const float* eys,
                                              int32_t only_stereo, int32_t check_orientation, int32_t* match12, int32_t* nmatches);

/* a15  SearchForInitialization(Frame& F1, Frame& F2, vbPrevMatched, vnMatches12, windowSize) -- src/ORBmatcher.cc:405-520.
 * F1: n1 keypoints (octave, angle, descriptors); prev_matched: n1 x 2 floats, updated in place like vbPrevMatched. */
eao_status eao_search_for_initialization(int32_t n1, const int32_t* octave1, const float* angle1, const uint8_t* desc1,
                                         const eao_frame_view* F2, float* prev_matched, int32_t window, float nnratio,
                                         int32_t check_orientation, int32_t* match12, int32_t* nmatches);

/* a15  the search half of Fuse(KeyFrame*, const vector<MapPoint*>&, th) -- src/ORBmatcher.cc:825-975 (use_sim3 = 0:
 * pose = Rcw (9) | tcw (3) | Ow (3) as 15 floats; reads KF->inv_level_sigma2 and the stereo / monocular chi2 gates) and of
 * Fuse(KeyFrame*, cv::Mat Scw, vpPoints, th, vpReplacePoint) -- :977-1100 (use_sim3 = 1: pose = Scw, 16 floats).
 * best_kp[i] receives the keypoint the point would be fused into (best distance <= TH_LOW) or -1; replacing or adding the
 * observation is the caller's part (it mutates the map), in index order, re-checking isBad() as upstream would. */
eao_status eao_fuse_search(const eao_frame_view* KF, int32_t use_sim3, const float* pose, float fx, float fy, float cx, float cy,
                           float bf, const eao_map_points* pts, float th, int32_t* best_kp, int32_t* nfused);

/* The same points against ALL target keyframes of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:458-520 calls Fuse once per target) in one call: the
 * points travel once, every target's frame and windows in the same copy, one synchronisation.  KFs: n_kf pointers; poses: 15 (use_sim3 = 0) or 16 floats per
 * target; best_kp: n_kf x pts->n; nfused: n_kf.  Equal to n_kf single calls ON THE SAME MAP STATE: an earlier target's fusions change the map, so the caller,
 * applying the targets in order, re-checks isBad() and IsInKeyFrame(pKFi) (upstream's `continue`s, src/ORBmatcher.cc:851-861) before it uses a later
 * target's candidate -- and searches again, against the remaining targets, every point whose DESCRIPTOR an applied fusion changed (pMPinKF->Replace(pMP) ends in
 * pMP->ComputeDistinctiveDescriptors(), src/MapPoint.cc:177-215): eaofusion::ORBmatcher::FuseBatch does both. */
eao_status eao_fuse_search_batch(int32_t n_kf, const eao_frame_view* const* KFs, int32_t use_sim3, const float* poses, float fx, float fy, float cx, float cy,
                                 float bf, const eao_map_points* pts, float th, int32_t* best_kp, int32_t* nfused);

/* a15  SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) -- src/ORBmatcher.cc:1102-1326.  pts1 / pts2: the map
 * points of the two keyframes by keypoint index (active = exists, not bad, not already matched); T1w / T2w: 16 floats.
 * match12[i] = keypoint of KF2 whose map point agrees in both directions, or -1 (already matched entries are not touched
 * by the caller). */
eao_status eao_search_by_sim3(const eao_frame_view* K1, const float* T1w, const eao_map_points* pts1, const eao_frame_view* K2,
                              const float* T2w, const eao_map_points* pts2, float fx, float fy, float cx, float cy, float s12,
                              const float* R12, const float* t12, float th, int32_t* match12, int32_t* nfound);

/* ---- keyframe handles (round 5): upload once, search many -------------------------------------------------------------------
 * LocalMapping::CreateNewMapPoints / SearchInNeighbors (reference src/LocalMapping.cc:211-290, 458-520) and LoopClosing search the SAME keyframes again and
 * again; the entry points above upload every frame with every call.  An eao_keyframe keeps what the guided searches read of a KeyFrame -- or of a Frame that is
 * a search target -- in HBM: the view's keypoints / octaves / angles / uRight / descriptors, the grid order GetFeaturesInArea walks (built once), the scale
 * tables, the DBoW2 feature vector (fv, may be NULL: the handle then serves the window searches only) and the occupancy view->occupied (NULL = none).  The
 * arrays are copied: the caller's may go away.  A handle is immutable but for its occupancy; searches only read it, so any number of threads may search the
 * same handle (each thread has its own stream and scratch).  `_kf` variants return exactly what their host-array counterparts above return on the same data. */
typedef struct eao_keyframe eao_keyframe;
eao_status eao_keyframe_create(const eao_frame_view* view, const eao_feature_vector* fv, eao_keyframe** out);
/* occupied[k] != 0 where the keyframe holds a map point at keypoint k (GetMapPoint(k) != NULL) -- what SearchForTriangulation skips on both sides
 * (src/ORBmatcher.cc:696-700, 712-716); NULL = no keypoint occupied.  Call it when map points were added to / erased from the keyframe -- from the thread that owns the
 * keyframe's map points (LocalMapping), and not while another thread searches this handle: the update is the one writer, ordered by the caller like upstream's mMutexFeatures. */
eao_status eao_keyframe_update_points(eao_keyframe* kf, const uint8_t* occupied);
void eao_keyframe_destroy(eao_keyframe* kf);
int32_t eao_keyframe_size(const eao_keyframe* kf);      /* number of keypoints, -1 for NULL */

/* a14 on handles, selection included ON THE DEVICE (a wavefront per common vocabulary node; two launches, one small copy back): arguments as
 * eao_search_by_bow.  valid1 / valid2 change with the map and travel per call (n bytes each). */
eao_status eao_kf_search_by_bow(int32_t mode, const eao_keyframe* kf1, const uint8_t* valid1, const eao_keyframe* kf2, const uint8_t* valid2, float nnratio,
                                int32_t check_orientation, int32_t* match12, int32_t* nmatches);
/* a15 on handles, all neighbours of LocalMapping::CreateNewMapPoints in one call, selection on the device: arguments as eao_search_for_triangulation_batch
 * (n_nb = 1: the single search); the occupancy of both sides is the handles' (eao_keyframe_update_points).  match12: n_nb x size(kf1). */
eao_status eao_kf_search_for_triangulation(const eao_keyframe* kf1, int32_t n_nb, const eao_keyframe* const* kf2s, const float* F12s, const float* exs,
                                           const float* eys, int32_t only_stereo, int32_t check_orientation, int32_t* match12, int32_t* nmatches);
/* a15 on handles, all targets of LocalMapping::SearchInNeighbors (or one: n_kf = 1) in one call: projection, window walk and gated best candidate per
 * (target, point) on the device; arguments as eao_fuse_search_batch.  The points change from call to call and travel each time (70 bytes per point). */
eao_status eao_kf_fuse_search(int32_t n_kf, const eao_keyframe* const* kfs, int32_t use_sim3, const float* poses, float fx, float fy, float cx, float cy,
                              float bf, const eao_map_points* pts, float th, int32_t* best_kp, int32_t* nfused);
/* a13 / a15: the list-based searches with the searched frame taken from a handle (only the queries travel; the selection is replayed on the host as before).
 * `occupied` replaces view->occupied of the host-array form (it differs from search to search: vpMatched, CurrentFrame.mvpMapPoints); NULL = none. */
eao_status eao_kf_search_by_projection_sim3(const eao_keyframe* kf, const uint8_t* occupied, const float* Scw, float fx, float fy, float cx, float cy,
                                            const eao_map_points* pts, int32_t th, int32_t* kp_match, int32_t* nmatches);
eao_status eao_kf_search_by_projection_kf(const eao_keyframe* cur, const uint8_t* occupied, const float* Tcw, float fx, float fy, float cx, float cy,
                                          const eao_map_points* pts, const float* kf_angle, float th, int32_t orb_dist, int32_t check_orientation,
                                          int32_t* cur_match, int32_t* nmatches);
eao_status eao_kf_search_for_initialization(int32_t n1, const int32_t* octave1, const float* angle1, const uint8_t* desc1, const eao_keyframe* f2,
                                            float* prev_matched, int32_t window, float nnratio, int32_t check_orientation, int32_t* match12, int32_t* nmatches);
eao_status eao_kf_search_by_sim3(const eao_keyframe* k1, const float* T1w, const eao_map_points* pts1, const eao_keyframe* k2, const float* T2w,
                                 const eao_map_points* pts2, float fx, float fy, float cx, float cy, float s12, const float* R12, const float* t12, float th,
                                 int32_t* match12, int32_t* nfound);

/* ---- the second half of LocalMapping::CreateNewMapPoints: triangulate and gate the matched pairs -- src/LocalMapping.cc:288-454 ----
 * Per matched pair (idx1 of the current keyframe, idx2 = match12[idx1] of a neighbour): the parallax test and the branch choice (:303-353: linear
 * triangulation, KeyFrame::UnprojectStereo of keyframe 1 or 2 -- src/KeyFrame.cc:654-670 --, or "no stereo and very low parallax"), then the gates of
 * :355-435 in upstream's order.  One verdict per slot of the match table; creating the MapPoint and its observations (:437-453) stays with the caller.
 * Arithmetic: cv::Mat products, dot and norm accumulate in double in storage order and round once; the chi2 gates compare
 * 5.991 * sigma2 / 7.8 * sigma2 in double against the float sum; the singular vector comes from a cyclic Jacobi solve in double on A^T A (fixed sweeps). */
typedef enum {
    EAO_TRI_EMPTY = 0,           /* match12 slot is -1: no pair, no point */
    EAO_TRI_TRIANGULATED = 1,    /* accepted, linear triangulation (:324-343) */
    EAO_TRI_UNPROJECTED_1 = 2,   /* accepted, mpCurrentKeyFrame->UnprojectStereo(idx1) (:344-347) */
    EAO_TRI_UNPROJECTED_2 = 3,   /* accepted, pKF2->UnprojectStereo(idx2) (:348-351) */
    EAO_TRI_LOW_PARALLAX = 4,    /* "No stereo and very low parallax" (:352-353); no point */
    EAO_TRI_W_ZERO = 5,          /* x3D.at<float>(3) == 0 (:337); no point */
    EAO_TRI_BEHIND_1 = 6,        /* z1 <= 0 (:359) */
    EAO_TRI_BEHIND_2 = 7,        /* z2 <= 0 (:363) */
    EAO_TRI_REPROJ_1 = 8,        /* reprojection gate in keyframe 1 (:372-391) */
    EAO_TRI_REPROJ_2 = 9,        /* reprojection gate in keyframe 2 (:398-417) */
    EAO_TRI_ZERO_DIST = 10,      /* dist1 == 0 || dist2 == 0 (:426) */
    EAO_TRI_SCALE = 11,          /* scale consistency (:434) */
    EAO_TRI_NO_DEPTH = 12        /* an unprojection branch met !(depth > 0): upstream would dereference the empty Mat UnprojectStereo returns; here no point */
} eao_tri_verdict;
/* verdicts 1..3 accept.  x3d of a rejected slot is left as computed when the point existed (verdicts 6..11) and is zero when it did not (0, 4, 5, 12). */

/* What the loop reads of a keyframe's pose and camera: GetRotation() (row-major), GetTranslation(), GetCameraCenter() as the caller's KeyFrame returns them
 * (Rwc is the transpose of Rcw, the translation of Twc is Ow), and fx, fy, cx, cy, invfx, invfy, mb, mbf. */
typedef struct {
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
} eao_tri_camera;

/* Host arrays, all neighbours in one call (src/LocalMapping.cc:288-454 over the tables eao_search_for_triangulation_batch returns).  K1 / K2s: the views'
 * kp_x, kp_y, kp_octave, u_right, scale_factors, level_sigma2 are read; depth = mvDepth; raw_x / raw_y = mvKeys[i].pt, which KeyFrame::UnprojectStereo reads
 * instead of mvKeysUn (src/KeyFrame.cc:659-660) -- NULL: they equal kp_x / kp_y.  depth2s / raw_x2s / raw_y2s: n_nb pointers (raw_x2s / raw_y2s or single
 * entries of them may be NULL).  match12: n_nb x K1->n, -1 for an empty slot, otherwise an index below K2s[k]->n; ratio_factor = 1.5f * mfScaleFactor (:236).
 * verdict: n_nb x K1->n eao_tri_verdict codes; x3d: n_nb x K1->n x 3.  A malformed table or view fails with EAO_ERR_INVALID before anything is written. */
eao_status eao_triangulate_matches_batch(const eao_frame_view* K1, const eao_tri_camera* cam1, const float* depth1, const float* raw_x1, const float* raw_y1,
                                         int32_t n_nb, const eao_frame_view* const* K2s, const eao_tri_camera* cams2, const float* const* depth2s,
                                         const float* const* raw_x2s, const float* const* raw_y2s, const int32_t* match12, float ratio_factor,
                                         int32_t* verdict, float* x3d);

/* mvDepth and mvKeys[i].pt of a resident keyframe (raw_x / raw_y NULL: the handle's kp_x / kp_y), copied into the handle once like its other arrays.
 * depth: eao_keyframe_size(kf) floats.  Not while another thread searches this handle (as eao_keyframe_update_points). */
eao_status eao_keyframe_set_depth(eao_keyframe* kf, const float* depth, const float* raw_x, const float* raw_y);

/* CreateNewMapPoints over resident keyframes: the search of eao_kf_search_for_triangulation (same arguments, same match12 / nmatches byte for byte) and the
 * triangulation of eao_triangulate_matches_batch over its tables, on one stream with no host hop between them and one wait: the triangulation kernel reads
 * the match table where the selection kernel left it.  cams2: n_nb records.  Every handle needs its depth (eao_keyframe_set_depth): one without fails
 * with EAO_ERR_INVALID before anything is written. */
eao_status eao_kf_create_new_map_points(const eao_keyframe* kf1, const eao_tri_camera* cam1, int32_t n_nb, const eao_keyframe* const* kf2s,
                                        const eao_tri_camera* cams2, const float* F12s, const float* exs, const float* eys, int32_t only_stereo,
                                        int32_t check_orientation, float ratio_factor, int32_t* match12, int32_t* nmatches, int32_t* verdict, float* x3d);
/* Diagnostic (tools/bench_triangulation.py): with EAO_TRI_EVENTS=1 in the environment, the device time in ms of the triangulation launches of this thread's last
 * eao_kf_create_new_map_points, from HIP events on its stream.  An event call that fails costs that measurement
 * (-1 in its slot) and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_kf_last_triangulation_ms(float* ms);

/* ---- f1  Frame glue either side of the matcher ------------------------------------------------------------------ */

/* What Frame::isInFrustum reads of the frame: mTcw (16 floats row-major: mRcw, mtcw), mOw, the static intrinsics and image
 * bounds (fx, fy, cx, cy, mbf, mnMinX .. mnMaxY) and mfLogScaleFactor. */
typedef struct {
    float Tcw[16];
    float Ow[3];
    float fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;
    float log_scale_factor;
} eao_frustum_frame;

/* Frame::isInFrustum(MapPoint*, viewingCosLimit) -- src/Frame.cc:638-695 -- for every point of pts, i.e. the projection
 * loop of Tracking::SearchLocalPoints (src/Tracking.cc:2612-2626; the caller keeps its own skip rules: mnLastFrameSeen,
 * isBad()).  pts: Xw, normal, min_dist_inv / max_dist_inv (Get{Min,Max}DistanceInvariance()), max_dist (mfMaxDistance, the
 * numerator of MapPoint::PredictScale, src/MapPoint.cc:385-394 -- not clamped in this fork); active and desc are not read.
 * in_view[i] = the return value = mbTrackInView; proj_x / proj_y / proj_xr / view_cos / pred_level receive mTrackProjX,
 * mTrackProjY, mTrackProjXR, mTrackViewCos, mnTrackScaleLevel where in_view[i] = 1 and keep the caller's values elsewhere
 * (upstream leaves those members untouched).  The outputs are exactly the inputs of eao_search_by_projection_points. */
eao_status eao_frame_is_in_frustum(const eao_frustum_frame* F, const eao_map_points* pts, float viewing_cos_limit, uint8_t* in_view,
                                   float* proj_x, float* proj_y, float* proj_xr, float* view_cos, int32_t* pred_level);

/* Frame::AssignFeaturesToGrid() with PosInGrid -- src/Frame.cc:597-614, 751-761 -- over mvKeysUn.  mGrid comes back as a CSR:
 * cell c = ix * rows + iy is mGrid[ix][iy]; cell_start has cols * rows + 1 entries; items[cell_start[c] .. cell_start[c+1])
 * are the keypoint indices of the cell in push_back (= ascending) order.  items needs room for n entries. */
eao_status eao_assign_features_to_grid(int32_t n, const float* kp_x, const float* kp_y, float min_x, float min_y, float grid_inv_w,
                                       float grid_inv_h, int32_t cols, int32_t rows, int32_t* cell_start, int32_t* items);

/* Frame::ComputeStereoFromRGBD(imDepth) -- src/Frame.cc:1016-1037.  kp_x / kp_y: mvKeys[i].pt (distorted), kpu_x:
 * mvKeysUn[i].pt.x; depth: the CV_32F depth image (`pitch` floats per row), a host pointer or, with depth_on_device != 0,
 * a device pointer (a depth map that is already resident).  u_right / out_depth receive mvuRight / mvDepth (-1 where the
 * depth is not positive). */
eao_status eao_compute_stereo_from_rgbd(int32_t n, const float* kp_x, const float* kp_y, const float* kpu_x, const float* depth,
                                        int32_t width, int32_t height, int32_t pitch, int32_t depth_on_device, float mbf,
                                        float* u_right, float* out_depth);

/* Frame::UndistortKeyPoints() -- src/Frame.cc:773-806: mvKeysUn[i].pt = cv::undistortPoints(mvKeys[i].pt, mK, mDistCoef, cv::Mat(), mK) (OpenCV 3.x:
 * five fixed-point iterations of the inverse distortion model in double, result rounded to float).  dist_coef: mDistCoef as the reference fills it
 * (src/Tracking.cc:90-101): k1, k2, p1, p2 and, with n_coef == 5, k3.  dist_coef[0] == 0 (or n_coef == 0): the coordinates are copied, as upstream copies
 * mvKeys (:775-779).  One thread per keypoint on the device; host arrays in and out. */
eao_status eao_undistort_keypoints(int32_t n, const float* kp_x, const float* kp_y, float fx, float fy, float cx, float cy,
                                   const float* dist_coef, int32_t n_coef, float* out_x, float* out_y);
/* Frame::ComputeImageBounds(imLeft) -- src/Frame.cc:808-842: bounds = { mnMinX, mnMaxX, mnMinY, mnMaxY } from the undistorted image corners, clamped to
 * the image ("make sure it is inside image", :828-832). */
eao_status eao_compute_image_bounds(int32_t cols, int32_t rows, float fx, float fy, float cx, float cy, const float* dist_coef, int32_t n_coef,
                                    float* bounds);

/* f4  Frame::ComputeStereoMatches() -- src/Frame.cc:841-1013.  `left` / `right` are the two extractor handles
 * (mpORBextractorLeft / Right) right after they extracted the stereo pair: the image pyramids of frame `frame` of their
 * last batch are still on the device and are read in place (the 19-px reflect-101 border of mvImagePyramid is evaluated
 * on the fly).  kps / desc: mvKeys + mDescriptors and mvKeysRight + mDescriptorsRight.  mb, mbf: Frame::mb, mbf.
 * u_right[i] / depth[i] receive mvuRight / mvDepth (-1 = no match), after the median-based outlier rejection. */
eao_status eao_compute_stereo_matches(eao_orb* left, eao_orb* right, int32_t frame, int32_t nl, const eao_keypoint* kps_l,
                                      const uint8_t* desc_l, int32_t nr, const eao_keypoint* kps_r, const uint8_t* desc_r,
                                      float mb, float mbf, float* u_right, float* depth);

/* f4  MapPoint::ComputeDistinctiveDescriptors() -- src/MapPoint.cc:242-307, batched over map points.  Set s holds the
 * descriptors of the (non-bad) keyframes observing point s, in std::map<KeyFrame*, size_t> iteration order:
 * desc[32 * k] for set_start[s] <= k < set_start[s + 1].  best[s] receives the position inside the set of the descriptor
 * with the least median Hamming distance to the others (median = sorted[(int)(0.5 * (N - 1))], the distance to itself
 * included; first index wins ties), or -1 for an empty set. */
eao_status eao_distinctive_descriptors(int32_t n_sets, const int32_t* set_start, const uint8_t* desc, int32_t* best);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::PoseOptimization(Frame*) -- reference include/Optimizer.h:56, src/Optimizer.cc:325-673
 * (point / stereo edges and the plane edges of src/Optimizer.cc:456-535)
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n;               /* matched map points (pFrame->mvpMapPoints[i] != NULL), in index order */
    const float* Tcw;        /* 16 floats, row-major 4x4: pFrame->mTcw */
    const float* Xw;         /* n*3: MapPoint::GetWorldPos() */
    const float* obs;        /* n*3: mvKeysUn[i].pt.x, .pt.y, mvuRight[i]  (mvuRight < 0 => monocular edge) */
    const float* inv_sigma2; /* n: mvInvLevelSigma2[mvKeysUn[i].octave] */
    float fx, fy, cx, cy, bf;
    /* plane edges (src/Optimizer.cc:456-535, 626-658; src/g2oAddition/EdgePlane.h, Plane3D.h): one per associated map
     * plane (pFrame->mvpMapPlanes[i] != NULL), in index order; n_planes = 0 and NULL pointers when there are none */
    int32_t n_planes;           /* at most 32 */
    const float* plane_world;   /* n_planes*4: MapPlane::GetWorldPos() */
    const float* plane_obs;     /* n_planes*4: pFrame->mvPlaneCoefficients[i] */
    const uint8_t* plane_seen;  /* n_planes:   MapPlane::mbSeen (unseen planes get twice the information) */
} eao_pose_problem;

typedef struct {
    float Tcw[16];      /* optimised pose as Converter::toCvMat would deliver it */
    uint8_t* outlier;   /* n flags: pFrame->mvbOutlier (caller-allocated) */
    int32_t n_inliers;  /* return value of PoseOptimization: nInitialCorrespondences - nBad */
    int32_t lm_iterations; /* outer LM iterations executed over the 4 rounds */
    uint8_t* plane_outlier; /* n_planes flags: pFrame->mvbPlaneOutlier (caller-allocated; may be NULL when n_planes = 0) */
} eao_pose_result;

eao_status eao_pose_optimization(const eao_pose_problem* p, eao_pose_result* r);

/* `n` independent PoseOptimization problems in one call: the candidate loop of Tracking::Relocalization
 * (reference src/Tracking.cc:2786-2940: the first Optimizer::PoseOptimization (:2885) of every candidate keyframe whose PnP converged)
 * and offline replays.  One workgroup per frame, one upload, one launch, one synchronisation; results[i] is
 * bit-identical to what eao_pose_optimization(&problems[i], &results[i]) returns.  Frames with more than 2048
 * correspondences are run one by one through that entry point. */
eao_status eao_pose_optimization_batch(const eao_pose_problem* problems, int32_t n, eao_pose_result* results);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*) -- reference include/Optimizer.h:55,
 * src/Optimizer.cc:675-1138.  The adapter flattens the local window: cameras in ascending KeyFrame::mnId
 * (free = lLocalKeyFrames, fixed = lFixedCameras or mnId == 0), points in ascending MapPoint::mnId, edges
 * in insertion order.  At most one edge per (camera, point).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_cams, n_points, n_edges;
    const float* cam_Tcw;         /* n_cams*16 */
    const uint8_t* cam_fixed;     /* n_cams */
    const float* points;          /* n_points*3 */
    const int32_t* edge_cam;      /* n_edges */
    const int32_t* edge_point;    /* n_edges */
    const float* edge_obs;        /* n_edges*3: u, v, ur (ur < 0 => monocular) */
    const float* edge_inv_sigma2; /* n_edges */
    float fx, fy, cx, cy, bf;
    int32_t its_first, its_second; /* 5 and 10 upstream (src/Optimizer.cc:966,1027) */
} eao_ba_problem;

typedef struct {
    float* cam_Tcw;        /* n_cams*16 out */
    float* points;         /* n_points*3 out */
    uint8_t* edge_outlier; /* n_edges: observation to erase (chi2 > 5.991/7.815 or depth <= 0), src/Optimizer.cc:1040-1068 */
    int32_t iters[2];      /* outer LM iterations executed in the two passes */
    int32_t aborted;       /* 1 when *stop was set on entry (src/Optimizer.cc:961-963): outputs = inputs */
    double chi2[2];        /* robust chi2 after each pass */
} eao_ba_result;

/* stop may be NULL; it is polled on the host between LM iterations like g2o's forceStopFlag */
eao_status eao_local_ba(const eao_ba_problem* p, const volatile uint8_t* stop, eao_ba_result* r);

/* The same call for n INDEPENDENT windows at once (BASELINE configs[4]: the 25 local-BA windows of a batched sequence; in
 * a live system: the windows of several maps / agents).  Every window is exactly one eao_local_ba call -- same inputs, same
 * outputs, same LM schedule (src/Optimizer.cc:675-1138 per window; independence per SURVEY.md s8e) -- but the window is the
 * z dimension of every kernel launch, so one enqueue serves them all.  Windows the batched path does not take (more than 30
 * free keyframes, nothing to optimise) run one after the other inside the same call.  `stop` is shared by all windows.
 * eao_last_lm_timing then reports the device time of the whole batch and the linearisations summed over the windows. */
eao_status eao_local_ba_batch(const eao_ba_problem* problems, int32_t n, const volatile uint8_t* stop, eao_ba_result* results);

/* f3  Optimizer::BundleAdjustment(vpKFs, vpMP, vpMPl, nIterations, pbStopFlag, nLoopKF, bRobust) --
 * src/Optimizer.cc:55-323: the same flattening as eao_local_ba (cameras in ascending mnId with
 * cam_fixed = (mnId == 0), points in ascending mnId, points without an edge simply stay where they are),
 * ONE optimize(p->its_first) call (its_second is ignored), Huber kernels (delta sqrt(5.99) / sqrt(7.815), :94-95) only
 * when robust != 0, no outlier pass: r->edge_outlier may be NULL and comes back all zero, r->iters[1] = 0.
 * Up to 30 free keyframes run on the register-tile solver of eao_local_ba; beyond that (whole maps after a loop
 * closure, up to 8192 free keyframes) the reduced camera system is kept as block-sparse 64 x 64 tiles in HBM, in a nested-dissection
 * order, and factorised by the whole chip (csrc/gba.hip, k_bal_*); oversized windows of eao_local_ba take the same path. */
eao_status eao_bundle_adjustment(const eao_ba_problem* p, int32_t robust, const volatile uint8_t* stop, eao_ba_result* r);

/* The MapPlane vertices / EdgePlane edges of the same function (src/Optimizer.cc:203-252; src/g2oAddition/VertexPlane.h,
 * EdgePlane.h, Plane3D.h): every non-bad map plane is a marginalised 3-dof vertex (Plane3D::oplus), every observation by
 * a keyframe of the graph an edge with information diag(3282.8, 3282.8, 1e4), ALWAYS a Huber kernel (delta sqrt(300))
 * and g2o's numeric Jacobians on both vertices.  planes == NULL or n_planes == 0: same as eao_bundle_adjustment. */
typedef struct {
    int32_t n_planes;
    const float* plane_world;     /* n_planes*4: MapPlane::GetWorldPos() */
    int32_t n_pedges;
    const int32_t* pedge_plane;   /* n_pedges: index into plane_world */
    const int32_t* pedge_cam;     /* n_pedges: index into p->cam_Tcw */
    const float* pedge_obs;       /* n_pedges*4: KeyFrame::mvPlaneCoefficients[observation index] */
} eao_ba_planes;
eao_status eao_bundle_adjustment_planes(const eao_ba_problem* p, const eao_ba_planes* planes, int32_t robust, const volatile uint8_t* stop,
                                        eao_ba_result* r, float* planes_out /* n_planes*4: Converter::toCvMat(vPlane->estimate()) */);

/* (diagnostic, host only -- needs no device) The elimination order, tile structure and launch schedule the map-scale path derives from a covisibility pattern
 * (round 6; csrc/gba.hip gba_build_plan: one level of nested dissection of the keyframe graph, the block form of the symbolic phase of the reference's
 * SimplicialLDLT + AMD ordering, Thirdparty/g2o/g2o/solvers/linear_solver_eigen.h:95-112).  pair_a[k] <= pair_b[k]: the covisible pairs of the n_free free keyframes,
 * the diagonal pairs (i, i) included.  force_segments: 0 = the library's choice, 1 = natural order, p > 1 = p segments.  Arrays the caller passes as NULL (or whose
 * capacity is too small) are left out; `info` always comes back, so a second call can size them.  tests/test_gba_plan.py replays the schedule on the CPU against a
 * dense solve. */
typedef struct {
    int32_t n_free, n_rows /* N: padded system, a multiple of 64; row N = the right-hand side */, n_tile_rows /* T = N / 64 + 1 */, n_panels /* N / 32 */, n_tiles;
    int32_t n_segments, n_separator, separator_start /* first row of the separator block */, rcm /* 1: the line is a reverse Cuthill-McKee order */, bandwidth;
    int32_t chain_natural /* factorisation launches of the natural order */, chain_estimate /* this plan's launches, factorisation + back substitution */;
    int32_t n_launches, n_work /* record pairs */, n_diag, n_sb, n_sb_launches;
} eao_gba_plan_info;
eao_status eao_bundle_adjustment_plan(int32_t n_free, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, int32_t force_segments, eao_gba_plan_info* info,
                                      int32_t* row_of /* n_free */, int32_t* tile_map /* T * T */, int32_t cap_tile_map, int32_t* work /* 8 per record pair */, int32_t cap_work,
                                      int32_t* launches /* 4 each: work offset, count, diag offset, count */, int32_t cap_launches, int32_t* diag_list, int32_t cap_diag,
                                      int32_t* sb /* 4 each: first column, width, chunk lo, chunk hi */, int32_t cap_sb, int32_t* sb_launches /* 3 each: offset, count, grid.x */,
                                      int32_t cap_sb_launches);

/* LM trace of the last eao_local_ba / eao_pose_optimization call made by this thread (for parity tests):
 * up to cap entries of (lambda after the iteration, robust chi2, trials). Returns the count in *n. */
eao_status eao_last_lm_trace(double* lambda, double* chi2, int32_t* trials, int32_t cap, int32_t* n);

/* PoseOptimization runs up to four optimize() calls (rounds, src/Optimizer.cc:541-660) and lays their traces end to end.  Frame `frame` of the last
 * eao_pose_optimization (frame 0) / eao_pose_optimization_batch call made by this thread: its trace as eao_last_lm_trace gives it, the number of
 * rounds it ran in *n_rounds and the trace index at which each began in round_start[0 .. 4) (-1 for a round that was not run; a round without an
 * iteration begins where the next one does). */
eao_status eao_last_pose_rounds(int32_t frame, double* lambda, double* chi2, int32_t* trials, int32_t cap, int32_t* n, int32_t* round_start, int32_t* n_rounds);

/* HIP-event time (ms) spent in device work by the last eao_local_ba / eao_pose_optimization on this thread,
 * and the number of linearisations (buildSystem calls) it made. */
eao_status eao_last_lm_timing(float* device_ms, int32_t* linearizations);

/* ---- f1, second half: the device-resident tracked frame ------------------------------------------------------------
 * Tracking::TrackLocalMap's data path (reference src/Tracking.cc:1717-2231, 2587-2641) chained on the device: the
 * extractor's device outputs of ONE frame go through Frame::ComputeStereoFromRGBD + AssignFeaturesToGrid (src/Frame.cc:
 * 599-614, 751-761, 1016-1037), Frame::isInFrustum over the local map (:638-695; viewingCosLimit 0.5 as in
 * Tracking::SearchLocalPoints), ORBmatcher::SearchByProjection(Frame&, local map points, th) (src/ORBmatcher.cc:45-137)
 * and Optimizer::PoseOptimization (src/Optimizer.cc:325-673, point edges) without returning to the host in between; one
 * copy brings back the pose, mvpMapPoints, mvbOutlier (and mvuRight / mvDepth).  Results are those of the host-hop calls
 * eao_compute_stereo_from_rgbd -> eao_frame_is_in_frustum -> eao_search_by_projection_points -> eao_pose_optimization on
 * the same data, bit for bit (tests/test_gpu_track.py).  Distortion-free camera (mvKeysUn = mvKeys), as the reference's
 * RGB-D configuration (ros_test/config/TUM3.yaml:13-16). */
typedef struct eao_tracker eao_tracker;
typedef struct {
    float fx, fy, cx, cy, mbf;                 /* Frame::fx .. mbf */
    float min_x, max_x, min_y, max_y;          /* mnMinX .. mnMaxY */
    int32_t grid_cols, grid_rows;              /* FRAME_GRID_COLS x FRAME_GRID_ROWS = 64 x 48 (include/Frame.h:89-90) */
    int32_t nlevels;
    const float* scale_factors;                /* nlevels: mvScaleFactors (copied) */
    const float* inv_level_sigma2;             /* nlevels: mvInvLevelSigma2 (copied) */
    float log_scale_factor;                    /* mfLogScaleFactor */
    int32_t max_keypoints;                     /* per frame, <= 4096; >= eao_orb_max_keypoints of the extractor */
    int32_t max_map_points;                    /* of a local map, <= 16384 */
} eao_tracker_cfg;
eao_status eao_tracker_create(const eao_tracker_cfg* cfg, eao_tracker** out);
void eao_tracker_destroy(eao_tracker* h);
/* The local map (Tracking::mvpLocalMapPoints) as plain arrays; uploaded once and kept in HBM until replaced.  active[i] = 0
 * where upstream skips the point (isBad()). */
eao_status eao_tracker_set_local_map(eao_tracker* h, const eao_map_points* pts);
typedef struct {
    float Tcw[16];            /* the optimised pose (the prior when fewer than 3 correspondences, src/Optimizer.cc:453-454) */
    int32_t n_keypoints;      /* N of the frame */
    int32_t n_matches;        /* return value of SearchByProjection */
    int32_t n_edges;          /* nInitialCorrespondences of PoseOptimization */
    int32_t n_inliers;        /* its return value */
    int32_t* kp_map_point;    /* caller array [max_keypoints]: mvpMapPoints as map-point index or -1 */
    uint8_t* kp_outlier;      /* caller array [max_keypoints]: mvbOutlier */
    float* kp_u_right;        /* optional caller arrays [max_keypoints]: mvuRight, mvDepth (NULL: not copied) */
    float* kp_depth;
    uint8_t* map_in_view;     /* optional caller array [max_map_points] (NULL: not copied): Frame::isInFrustum(pMP, 0.5) of every ACTIVE
                               * local map point -- what Tracking::SearchLocalPoints needs for IncreaseVisible() (src/Tracking.cc:2621-2625);
                               * the caller ignores the entries of points a prior match names (upstream never projects those) */
} eao_track_result;
/* d_kps / d_desc / d_n: ONE frame's slice of the device outputs of eao_orb_extract_batch_device (d_n points at that frame's
 * count); d_depth: the float depth image on the device (rows of depth_pitch floats) or NULL (monocular: mvuRight = -1);
 * Tcw_prior: the pose the frame enters TrackLocalMap with; prior_kp_map_point: mvpMapPoints as it stands (host array
 * [max_keypoints], NULL = none) -- those keypoints are occupied, their map points are not searched again, and they are
 * edges of the pose optimisation.  Entries: -1 = no map point; m in [0, n) = point m of the local map -- if that point is
 * inactive (isBad()) the prior is DROPPED and the keypoint is free, as upstream sets such an entry to NULL
 * (src/Tracking.cc:2596-2599), and the returned kp_map_point shows it; -2 = a map point that is not in the local map
 * (a temporal point of the RGB-D odometry, a point the local map lost): the keypoint stays occupied and its edge is built
 * from prior_kp_Xw[3k..3k+2] (host array [3 * max_keypoints], may be NULL when no entry is -2), kp_map_point returns -2;
 * anything else (an index >= n, e.g. a table older than the last eao_tracker_set_local_map) fails with EAO_ERR_INVALID before
 * any kernel runs.  `stream`: the stream the extraction was enqueued on -- the chain is enqueued on
 * that stream itself (ordered behind the extraction without an event hand-over); the call returns when the results are on the host. */
eao_status eao_tracker_track_local_map(eao_tracker* h, const eao_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                       const float* d_depth, int32_t depth_pitch, int32_t width, int32_t height, const float* Tcw_prior,
                                       const int32_t* prior_kp_map_point, const float* prior_kp_Xw, float th, float nnratio, eao_track_result* out,
                                       void* stream);

/* One-shot options of the NEXT eao_tracker_track_* call on the handle (round 5; NULL or never called: defaults).
 *  - plane edges (the association itself: eao_plane_map_associate, "MapPlane boundaries" below): in this fork Map::AssociatePlanesByBoundary runs BEFORE Optimizer::PoseOptimization in all three stages (src/Tracking.cc:1587, before :2181,
 *    TrackLocalMap), so the frame's associated planes are edges of the optimisation (src/Optimizer.cc:456-535, 626-658).  A caller whose frame carries them
 *    hands them over exactly as in eao_pose_problem (n_planes <= 32; plane_world = MapPlane::GetWorldPos(), plane_obs = mvPlaneCoefficients[i], plane_seen =
 *    mbSeen) and gets mvbPlaneOutlier back in plane_outlier (caller array, valid until the track call returns); the chained pose optimisation is then the
 *    plane instantiation of the same kernel -- same result as eao_pose_optimization with those planes on the chain's correspondences.
 *  - min_matches (motion-model / reference-keyframe stages): when the search returns fewer matches, the pose optimisation and the outlier discard are
 *    SKIPPED -- upstream repeats the search with 2 * th (src/Tracking.cc:1756-1763) or returns false (:1580-1581) before it optimises anything; the result then
 *    carries the search's tables, n_edges = n_inliers = 0 and the prior pose, and the caller touches no map point.  0 = always optimise. */
typedef struct {
    int32_t min_matches;
    int32_t n_planes;
    const float* plane_world;      /* n_planes*4 */
    const float* plane_obs;        /* n_planes*4 */
    const uint8_t* plane_seen;     /* n_planes */
    uint8_t* plane_outlier;        /* out: n_planes */
} eao_track_options;
eao_status eao_tracker_set_options(eao_tracker* h, const eao_track_options* opt);
/* The camera's lens distortion (mDistCoef; round 5).  With a non-zero k1 the frame set-up of every eao_tracker_track_* call undistorts the keypoints on the
 * device first (Frame::UndistortKeyPoints, as eao_undistort_keypoints): mvuRight, the grid, the searches and the pose edges then read mvKeysUn, the depth image
 * is looked up at the DISTORTED keypoint -- upstream's own split (src/Frame.cc:1016-1037).  cfg.min_x .. max_y are the caller's mnMinX .. mnMaxY
 * (eao_compute_image_bounds).  Persistent for the handle; n_coef == 0 or dist_coef[0] == 0: distortion-free (the default). */
eao_status eao_tracker_set_distortion(eao_tracker* h, const float* dist_coef, int32_t n_coef);

/* Tracking::TrackWithMotionModel's data path (reference src/Tracking.cc:1717-2231) on the same chain, ahead of TrackLocalMap: the frame set-up as
 * above, ORBmatcher::SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) (src/ORBmatcher.cc:1328-1472, with this fork's rotation-histogram
 * factor HISTO_LENGTH / 360, :1337) against the LAST frame's map points, Optimizer::PoseOptimization from the predicted pose, and -- when
 * discard_outliers != 0 -- the "Discard outliers" loop of src/Tracking.cc:2188-2207; one copy back.  The last frame travels as host arrays per
 * last-frame keypoint i (n_last <= max_keypoints entries): valid[i] != 0 where mvpMapPoints[i] != NULL && !mvbOutlier[i]; Xw = GetWorldPos();
 * mp_desc = GetDescriptor() (32 bytes); last_octave = mvKeys[i].octave; last_angle = mvKeysUn[i].angle.  Tcw_cur: the predicted pose
 * (mVelocity * mLastFrame.mTcw, :1726), Tcw_last: mLastFrame.mTcw; 16 floats row-major each, finite (EAO_ERR_INVALID otherwise).
 * Result (zero-initialise the struct and set the array pointers; map_in_view is not written): kp_map_point[k] = the LAST-FRAME INDEX whose map point
 * keypoint k took, or -1; n_matches = the search's return value (what upstream tests against 20 before it retries with 2 th -- the caller repeats the
 * call); n_edges = correspondences of the pose optimisation; n_inliers = n_edges minus the outliers = the matches left after the discard;
 * kp_outlier = mvbOutlier after PoseOptimization (all zero after the discard).  A keypoint a point has taken counts as occupied for the points behind
 * it, as for map points with Observations() > 0 (the same rule eao_search_by_projection_frames applies).  Same results as
 * eao_compute_stereo_from_rgbd -> eao_search_by_projection_frames -> eao_pose_optimization on the same data. */
eao_status eao_tracker_track_with_motion_model(eao_tracker* h, const eao_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                               const float* d_depth, int32_t depth_pitch, int32_t width, int32_t height, const float* Tcw_cur,
                                               const float* Tcw_last, int32_t n_last, const uint8_t* valid, const float* Xw, const uint8_t* mp_desc,
                                               const int32_t* last_octave, const float* last_angle, float th, int32_t mono, int32_t check_orientation,
                                               int32_t discard_outliers, eao_track_result* out, void* stream);

/* Tracking::TrackReferenceKeyFrame's data path (reference src/Tracking.cc:1568-1631) on the same chain: the frame set-up as above,
 * ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (src/ORBmatcher.cc:159-288: ORBmatcher(0.7, true) at :1574, rotation-histogram factor
 * 1 / HISTO_LENGTH :171), Optimizer::PoseOptimization from the last frame's pose (:1584-1590), and -- when discard_outliers != 0 -- the "Discard outliers" loop
 * (:1593-1612); one copy back.  The reference keyframe travels as host arrays per keyframe keypoint i (n_kf <= max_keypoints entries): valid[i] != 0 where
 * GetMapPointMatches()[i] != NULL && !isBad(); Xw = GetWorldPos(); kf_desc = pKF->mDescriptors.row(i); kf_angle = pKF->mvKeysUn[i].angle.  fv_kf = pKF->mFeatVec,
 * fv_cur = mCurrentFrame.mFeatVec: the frame's own vector is what Frame::ComputeBoW (:1571) makes of its descriptors -- this entry point
 * takes it as host arrays, so this stage still costs one trip to the host before the call (eao_vocabulary_transform_device computes the vector from the
 * descriptors in HBM; feeding it to this chain without the hop is a later change).  A keypoint index lies in ONE node (DBoW2 files a feature
 * under its single ancestor at levelsup); a vector that lists an index twice, out of range, or whose node ids do not ascend fails with EAO_ERR_INVALID before
 * any kernel runs, an index of fv_cur beyond the *d_n keypoints the extractor left fails after the chain.  Tcw_last: mLastFrame.mTcw, 16 floats row-major, finite.
 * Result as for eao_tracker_track_with_motion_model, with kp_map_point[k] = the KEYFRAME KEYPOINT INDEX whose map point frame keypoint k took, or -1, and n_matches =
 * SearchByBoW's return value (what upstream tests against 15 / 10).  Same results as eao_compute_stereo_from_rgbd -> eao_search_by_bow(mode 0) ->
 * eao_pose_optimization on the same data. */
eao_status eao_tracker_track_reference_keyframe(eao_tracker* h, const eao_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                                const float* d_depth, int32_t depth_pitch, int32_t width, int32_t height, const float* Tcw_last,
                                                int32_t n_kf, const uint8_t* valid, const float* Xw, const uint8_t* kf_desc, const float* kf_angle,
                                                const eao_feature_vector* fv_kf, const eao_feature_vector* fv_cur, float nnratio, int32_t check_orientation,
                                                int32_t discard_outliers, eao_track_result* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) -- reference include/Optimizer.h,
 * src/Optimizer.cc:1437-1632 (g2o: types/types_seven_dof_expmap.h:48-170, types/sim3.h:70-141, core/base_binary_edge.hpp:147-196,
 * core/optimization_algorithm_levenberg.cpp:61-189, solvers/linear_solver_dense.h:104-112)
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n;                  /* correspondences that got an edge pair (src/Optimizer.cc:1502-1561: vpMatches1[i] != NULL, pMP1 = GetMapPointMatches()[i]
                                 * != NULL, neither isBad(), pMP2->GetIndexInKeyFrame(pKF2) >= 0), in index order */
    const float* T1w;           /* 16 floats, row-major 4x4: pKF1 pose (GetRotation() = upper-left 3x3, GetTranslation() = last column) */
    const float* T2w;           /* 16 floats: pKF2 */
    const float* Xw1;           /* n*3: pMP1->GetWorldPos() */
    const float* Xw2;           /* n*3: pMP2->GetWorldPos() */
    const float* obs1;          /* n*2: pKF1->mvKeysUn[i].pt.x, .pt.y */
    const float* obs2;          /* n*2: pKF2->mvKeysUn[i2].pt.x, .pt.y */
    const float* inv_sigma2_1;  /* n: pKF1->mvInvLevelSigma2[mvKeysUn[i].octave] */
    const float* inv_sigma2_2;  /* n: pKF2->mvInvLevelSigma2[mvKeysUn[i2].octave] */
    float fx1, fy1, cx1, cy1;   /* pKF1->mK */
    float fx2, fy2, cx2, cy2;   /* pKF2->mK */
    double q[4];                /* the initial g2oS12: rotation coefficients in Eigen's order x, y, z, w */
    double t[3];                /*   translation */
    double s;                   /*   scale */
    float th2;                  /* chi2 gate of both inlier passes; the Huber width is sqrtf(th2) (src/Optimizer.cc:1495) */
    int32_t fix_scale;          /* bFixScale: VertexSim3Expmap::_fix_scale (the update's 7th component is zeroed) */
} eao_sim3_problem;

typedef struct {
    double q[4], t[3], s;       /* the optimised g2oS12 as the vertex holds it (x, y, z, w; t; s); the initial one on early exit */
    uint8_t* removed;           /* n flags (caller-allocated): 1 where the reference sets vpMatches1[i] = NULL, in either inlier pass */
    int32_t n_inliers;          /* return value of OptimizeSim3 (0 on early exit) */
    int32_t lm_iterations[2];   /* outer LM iterations of the two optimize() calls (the second is 0 on early exit) */
    int32_t early_exit;         /* 1: nCorrespondences - nBad < 10 after the first pass (src/Optimizer.cc:1591-1592), g2oS12 not written back */
} eao_sim3_result;

/* Camera-frame points R1w * Xw1 + t1w (src/Optimizer.cc:1525-1526, float cv::Mat): the product accumulates in double and rounds
 * once to float, the translation is added in float, then the result is promoted to double.  One workgroup runs both optimize()
 * calls, the inlier pass between them and the final one. */
eao_status eao_optimize_sim3(const eao_sim3_problem* p, eao_sim3_result* r);

/* `n` independent OptimizeSim3 problems in one launch (one workgroup per problem): offline replays, several maps or
 * candidates at once.  results[i] is bit-identical to what eao_optimize_sim3(&problems[i], &results[i]) returns. */
eao_status eao_optimize_sim3_batch(const eao_sim3_problem* problems, int32_t n, eao_sim3_result* results);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale) -- reference
 * include/Optimizer.h, src/Optimizer.cc:1141-1435: the Sim3 pose graph of LoopClosing::CorrectLoop (g2o: types/types_seven_dof_expmap.h:48-126,
 * types/sim3.h:70-230, core/base_binary_edge.hpp:147-196, core/optimization_algorithm_levenberg.cpp:61-189 with lambda0 = 1e-16,
 * solvers/linear_solver_eigen.h:95-125).  Keyframes carry a dense index 0 .. n-1 (the adapter compacts mnId).  A Sim3 is 8 doubles: the
 * rotation's coefficients in Eigen's order x, y, z, w, the translation, the scale.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n;                  /* keyframes that got a vertex (not isBad()) */
    int32_t fixed;              /* index of pLoopKF: the fixed vertex */
    int32_t fix_scale;          /* bFixScale: VertexSim3Expmap::_fix_scale */
    const double* Scw;          /* n*8: vScw -- CorrectedSim3 where the keyframe is in that map, else (GetRotation(), GetTranslation(), 1) */
    const uint8_t* has_nc;      /* n: 1 where the keyframe is in NonCorrectedSim3 */
    const double* Snc;          /* n*8: NonCorrectedSim3 (read where has_nc) */
    int32_t n_edges;
    const int32_t* edges;       /* n_edges*3: (i, j, kind), vertex 0 of the edge is i and vertex 1 is j, in the order upstream adds them.
                                 * kind 0 = loop connection: measurement vScw[j] * vScw[i]^-1; kind 1 = spanning tree / loop edge / covisibility:
                                 * the same with NonCorrectedSim3 in place of vScw where has_nc.  Duplicates all count. */
    int32_t n_points;
    const float* Xw;            /* n_points*3: GetWorldPos() of the good map points */
    const int32_t* ref;         /* n_points: index of the keyframe a point is corrected through (src/Optimizer.cc:1381-1390); -1: none, the point
                                 * comes back as it is */
} eao_essential_graph_problem;

typedef struct {
    double* Scw;                /* n*8 (caller-allocated): the optimised vertices; the fixed one and those without an edge bit-equal to the input */
    float* Tiw;                 /* n*16: toRotationMatrix() of the quaternion, t * (1 / s), rounded once to float (row-major 4x4) */
    float* Xw_corrected;        /* n_points*3: correctedSwr.map(Srw.map(X)) in double, rounded once to float */
    int32_t lm_iterations;      /* outer LM iterations of optimize(20) */
    int32_t trials[20];         /* per iteration: the trials it took, */
    double lambda[20];          /*   lambda as the iteration left it, */
    double chi2[20];            /*   chi2 of the estimate it ended with */
    double chi2_initial;
    int32_t n_active;           /* vertices with at least one edge (initializeOptimization() activates no other) */
} eao_essential_graph_result;

/* At most 8192 free keyframes with an edge (the capacity of eao_bundle_adjustment's map-scale solver, whose factor chain this runs on).
 * Non-finite input, `fixed` or an edge index out of range and an edge with i == j fail with EAO_ERR_INVALID before anything is written.
 * Two calls on the same problem return the same bytes. */
eao_status eao_optimize_essential_graph(const eao_essential_graph_problem* p, eao_essential_graph_result* r);

/* The elimination plan eao_optimize_essential_graph would solve this problem on (host only, no device needed; the same argument checks): the solver's
 * figures, row_of[n] = first of a keyframe's seven rows in the elimination order (-1: fixed or without an edge), tile_map[T * T] = slot of each 64 x 64 tile
 * of the lower triangle or -1 (copied when cap_tile_map is large enough; row_of and tile_map may be NULL). */
eao_status eao_essential_graph_plan(const eao_essential_graph_problem* p, eao_gba_plan_info* info, int32_t* row_of, int32_t* tile_map, int32_t cap_tile_map);

/* ------------------------------------------------------------------------------------------------
 * Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc): the Horn RANSAC of LoopClosing::ComputeSim3 (src/LoopClosing.cc:286-311),
 * between SearchByBoW and SearchBySim3.  One call is one Sim3Solver::iterate: its hypotheses are evaluated together (one wavefront each:
 * ComputeSim3 :226-337, CheckInliers :340-364), then the sequential part of the loop (:158-206) is replayed over their counts on the device.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n;                  /* correspondences that pass the constructor's filters (src/Sim3Solver.cc:62-102), in index order */
    const float* T1w;           /* 16 floats, row-major 4x4: pKF1 pose (GetRotation() / GetTranslation(), :54-55) */
    const float* T2w;           /* 16 floats: pKF2 (:56-57) */
    const float* Xw1;           /* n*3: pMP1->GetWorldPos() (:94) */
    const float* Xw2;           /* n*3: pMP2->GetWorldPos() (:97) */
    const float* sigma2_1;      /* n: pKF1->mvLevelSigma2[kp1.octave] (:84); finite, 0 <= sigma2 <= 1e12 */
    const float* sigma2_2;      /* n: pKF2->mvLevelSigma2[kp2.octave] (:85) */
    float fx1, fy1, cx1, cy1;   /* pKF1->mK (:105) */
    float fx2, fy2, cx2, cy2;   /* pKF2->mK (:106) */
    int32_t fix_scale;          /* mbFixScale */
} eao_sim3_solver_problem;

/* What survives between iterate calls (in/out).  A new solver starts from all zeros (SetRansacParameters :137, the constructor :38). */
typedef struct {
    int32_t iterations;         /* mnIterations */
    int32_t best_inliers;       /* mnBestInliers */
    float best_T12[16];         /* mBestT12, row-major 4x4 */
    float best_R[9];            /* mBestRotation */
    float best_t[3];            /* mBestTranslation */
    float best_s;               /* mBestScale */
} eao_sim3_solver_state;

typedef struct {
    int32_t returned;           /* position within the chunk of the hypothesis iterate returns (:192-199), or -1 */
    int32_t n_inliers;          /* nInliers (0 unless returned >= 0) */
    float T12[16];              /* the returned mBestT12 (zeros unless returned >= 0) */
    uint8_t* inlier;            /* n flags over the filtered correspondences (caller-allocated), written only when returned >= 0 */
    int32_t no_more;            /* bNoMore: n < min_inliers (:146-150; nothing is evaluated and the state is untouched), or
                                 * iterations >= max_its after the loop when nothing returned (:203-204) */
    /* inspection, each written when non-NULL; entries of hypotheses the call does not evaluate are zero */
    int32_t* hyp_inliers;       /* n_hyp: mnInliersi */
    float* hyp_T12;             /* n_hyp*16: mT12i */
    float* hyp_T21;             /* n_hyp*16: mT21i */
    uint8_t* hyp_inlier;        /* n_hyp*n: mvbInliersi */
} eao_sim3_solver_result;

/* Sim3Solver::iterate(n_hyp, ...) with mRansacMinInliers = min_inliers and mRansacMaxIts = max_its (the value SetRansacParameters :135 left).
 * triples: n_hyp*3 indices into 0 .. n-1 in draw order (:166-177); an index may repeat inside a triple (the sampling loop can produce
 * that), one out of range fails with EAO_ERR_INVALID before anything is written.  The first min(n_hyp, max_its - state->iterations)
 * hypotheses are evaluated; then, in order: one with inliers >= best_inliers becomes the best (a tie goes to the later one), and if its
 * inliers > min_inliers the call returns it -- iterations advances up to and including it, later hypotheses leave no trace in the state.
 * Arithmetic: float where upstream holds CV_32F, double where it holds double.  Camera-frame points as eao_optimize_sim3 makes them (the
 * product accumulates in double and rounds once to float, the translation is added in float); every small matrix product likewise; a double
 * scalar times a float matrix multiplies in double and rounds once; Mat::dot and cv::norm accumulate in double; the quaternion is the
 * eigenvector of a cyclic Jacobi solve in double, rounded to float.  The gate of correspondence i is (float)(size_t)(9.210 * sigma2[i])
 * (include/Sim3Solver.h:78-79 hold size_t).  Nothing is repaired: a zero imaginary part gives a NaN T12, a zero depth gives inf / NaN, and
 * a correspondence whose error is NaN is an outlier.  Two calls on the same arguments return the same bytes. */
eao_status eao_sim3_solver_iterate(const eao_sim3_solver_problem* problem, int32_t min_inliers, int32_t max_its, eao_sim3_solver_state* state,
                                   const int32_t* triples, int32_t n_hyp, eao_sim3_solver_result* result);

/* One round of ComputeSim3's round-robin over `n_problems` candidates (src/LoopClosing.cc:286-311) for an offline replay, in one launch chain:
 * problem b with min_inliers[b], max_its[b], states[b], triples[b] (n_hyp[b]*3 indices) and results[b].  Each result and state is
 * bit-identical to what eao_sim3_solver_iterate returns for it.  Any invalid problem fails the call before anything is written. */
eao_status eao_sim3_solver_iterate_batch(int32_t n_problems, const eao_sim3_solver_problem* problems, const int32_t* min_inliers, const int32_t* max_its,
                                         eao_sim3_solver_state* states, const int32_t* const* triples, const int32_t* n_hyp,
                                         eao_sim3_solver_result* results);

/* ------------------------------------------------------------------------------------------------
 * Initializer (reference include/Initializer.h, src/Initializer.cc): the homography / fundamental RANSAC and the two-view reconstruction of
 * Tracking::MonocularInitialization (src/Tracking.cc:1374-1392).  One call is Initializer::Initialize after its draws (:99-121): FindHomography
 * (:124-172) and FindFundamental (:175-223) over all sets at once, the choice of the model (:112-118), ReconstructH (:572-732) or ReconstructF
 * (:470-570) with CheckRT (:798-907) per motion hypothesis.
 * ------------------------------------------------------------------------------------------------ */
enum { EAO_INIT_BRANCH_H = 0, EAO_INIT_BRANCH_F = 1 };

typedef struct {
    int32_t n1, n2;             /* keypoints of the reference / the current frame (mvKeys1, mvKeys2: Frame::mvKeysUn) */
    const float* keys1_xy;      /* n1*2: pt.x, pt.y */
    const float* keys2_xy;      /* n2*2 */
    int32_t n_matches;          /* N = mvMatches12.size() (:49-63) */
    const int32_t* matches12;   /* N*2: (first, second), strictly ascending in `first` as the loop of :54-63 leaves them */
    float fx, fy, cx, cy;       /* mK */
    float sigma;                /* mSigma (> 0) */
    float min_parallax;         /* minParallax of ReconstructH / ReconstructF (upstream passes 1.0) */
    int32_t min_triangulated;   /* minTriangulated (upstream passes 50) */
} eao_initializer_problem;

typedef struct {
    int32_t returned;           /* what Initialize returns */
    int32_t branch;             /* EAO_INIT_BRANCH_H when RH > 0.40, else EAO_INIT_BRANCH_F */
    int32_t no_model;           /* the model of that branch has no hypothesis with a score above 0: returned = 0, nothing reconstructed */
    int32_t degenerate;         /* ReconstructH left through d1/d2 < 1.00001 || d2/d3 < 1.00001 (:597) */
    float SH, SF, RH;           /* the scores FindHomography / FindFundamental end with (0 without a winner) and SH/(SH+SF) */
    int32_t best_h, best_f;     /* the set whose hypothesis won (the first of equal scores), or -1 */
    float H21[9], F21[9];       /* the winners, row-major (zeros without one) */
    float R21[9], t21[3];       /* written when returned (zeros otherwise) */
    float parallax;             /* of the best motion hypothesis, degrees: acos(cos_parallax)*180/CV_PI formed on the host (0 without one) */
    float cos_parallax;         /* the sorted cosines' entry min(50, nGood-1) the device selected (1 when nGood = 0) */
    int32_t n_good;             /* nGood of the best motion hypothesis */
    int32_t motion;             /* its index among the 4 (F: (R1,t1) (R2,t1) (R1,t2) (R2,t2)) or 8 (H: vR / vt order), or -1 */
    int32_t n_motions;          /* 4, 8 or 0 (no_model, degenerate) */
    int32_t n_inliers;          /* N of ReconstructH / ReconstructF: set flags of the winner of the branch taken */
    float* p3d;                 /* n1*3 vP3D, caller-allocated; written only when returned (upstream leaves it alone otherwise) */
    uint8_t* triangulated;      /* n1 vbTriangulated, likewise */
    /* inspection, each written when non-NULL */
    float* hyp_H21;             /* iterations*9: H21i */
    float* hyp_H12;             /* iterations*9: H12i */
    float* hyp_F21;             /* iterations*9: F21i */
    float* hyp_SH;              /* iterations: currentScore of CheckHomography */
    float* hyp_SF;              /* iterations: currentScore of CheckFundamental */
    uint8_t* hyp_inlier_H;      /* iterations*N: vbCurrentInliers of CheckHomography (the only path that stores 2*iterations*N flags) */
    uint8_t* hyp_inlier_F;      /* iterations*N */
    uint8_t* inlier;            /* N: vbMatchesInliers of the branch taken */
    float* mot_R;               /* 8*9: the motion hypotheses (rows past n_motions are zero) */
    float* mot_t;               /* 8*3 */
    int32_t* mot_n_good;        /* 8: CheckRT's return */
    float* mot_cos;             /* 8: the selected cosine */
    uint8_t* mot_good;          /* 8*n1: vbGood */
    float* mot_p3d;             /* 8*n1*3: vP3D */
} eao_initializer_result;

/* sets: iterations*8 indices into 0 .. N-1, mvSets (:78-97) in draw order.  N >= 8, 1 <= iterations <= 65535, any n1, n2 >= 1 that fit the device.
 * EAO_ERR_INVALID before anything is written: N < 8, a set index >= N, a match index out of range or `first` not ascending, a non-finite keypoint
 * or intrinsic, sigma <= 0.
 * Arithmetic: upstream's float expressions op for op; OpenCV's by the conventions of eao_sim3_solver_iterate (small products accumulate in double
 * and round once, cv::norm / Mat::dot / cv::determinant in double, the 3 x 3 inverse by cofactors over a double determinant -- zero when singular);
 * every singular vector (the 16 x 9 and 8 x 9 systems of ComputeH21 :226-266 / ComputeF21 :268-303, the 3 x 3 SVDs, Triangulate's 4 x 4 :734-747)
 * is an eigenvector of A^T A in double from the float A, cyclic Jacobi with a fixed sweep count, rounded to float; its sign is not cv::SVD's, so the
 * 4 / 8 motion hypotheses agree with upstream's as a set, not by index.
 * Three deviations from upstream:
 *  1. A score (CheckHomography :305-388, CheckFundamental :390-468) is the sum of its terms in double, rounded once to float.  Every term is a float
 *     below 8 and a multiple of 2^-23, so that sum is exact: the same for every order, launch layout and run.  Upstream's float sum, term by term,
 *     differs from it by at most N * 2^-24 relative.
 *  2. no_model: upstream would throw from K.t()*F*K (or invK*H21*K) on the empty Mat.
 *  3. Normalize (:749-795) runs on the host inside this call, op for op, with upstream's sequential float sums over ALL keypoints of each frame.
 * Two calls on the same arguments return the same bytes. */
eao_status eao_initializer_initialize(const eao_initializer_problem* problem, const int32_t* sets, int32_t iterations, eao_initializer_result* result);

/* Diagnostic (tools/bench_initializer.py): with EAO_INIT_EVENTS=1 in the environment, the device time in ms of each of the five kernels of this thread's last
 * eao_initializer_initialize (hypotheses, scores, selection, CheckRT, final rule), from HIP events on its stream.  An event call that fails costs that measurement
 * (-1 in its slot) and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_initializer_last_kernel_ms(float* kernel_ms /* 5 */);

/* ------------------------------------------------------------------------------------------------
 * PnPsolver (reference include/PnPsolver.h, src/PnPsolver.cc): the EPnP RANSAC of Tracking::Relocalization (src/Tracking.cc:2786-2940), the step before
 * PoseOptimization.  One call is one PnPsolver::iterate (:165-258): compute_pose (:477-525) and CheckInliers (:308-339) of all its hypotheses together (one
 * wavefront each), the records among their counts, Refine (:260-305) of each record, then the sequential rule of the loop replayed on the device.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n;                  /* N: the correspondences the constructor keeps (:67-110), in index order */
    const float* p3d_w;         /* n*3: mvP3Dw */
    const float* p2d;           /* n*2: mvP2D */
    const float* sigma2;        /* n: mvSigma2 */
    float fx, fy, cx, cy;       /* F.fx .. F.cy; held in double from there on, as fu, fv, uc, vc are */
    float th2;                  /* the gate of correspondence i is the float sigma2[i] * th2 (:154-156) */
} eao_pnp_solver_problem;

/* What survives between iterate calls (in/out).  A new solver starts from all zeros (best_inlier: n zero bytes). */
typedef struct {
    int32_t iterations;         /* mnIterations */
    int32_t best_inliers;       /* mnBestInliers */
    float best_Tcw[16];         /* mBestTcw, row-major 4x4 */
    uint8_t* best_inlier;       /* n, caller-allocated: mvbBestInliers (Refine reads it across calls); exactly best_inliers of them are set */
} eao_pnp_solver_state;

typedef struct {
    int32_t returned;           /* -1: iterate returns an empty Mat.  refined = 1: the position in the chunk of the hypothesis whose Refine succeeded (:226-236).
                                 * refined = 0: the position of the best hypothesis (:241-254), or n_hyp when the state carried it in */
    int32_t refined;            /* which of the two return paths was taken (0 when nothing returns) */
    int32_t n_inliers;          /* nInliers (0 unless returned >= 0) */
    float Tcw[16];              /* the returned pose: the float rounding of the doubles (zeros unless returned >= 0) */
    uint8_t* inlier;            /* n flags over the correspondences (caller-allocated), written only when returned >= 0 */
    int32_t no_more;            /* bNoMore */
    int32_t n_records;          /* entries of the rec_* arrays */
    /* inspection, each written when non-NULL */
    double* hyp_R;              /* n_hyp*9: mRi of compute_pose over the sampled set */
    double* hyp_t;              /* n_hyp*3: mti */
    double* hyp_rep_err;        /* n_hyp*3: rep_errors[1..3] */
    int32_t* hyp_choice;        /* n_hyp: N of :518-520 */
    int32_t* hyp_inliers;       /* n_hyp: mnInliersi */
    uint8_t* hyp_inlier;        /* n_hyp*n: mvbInliersi */
    /* the sets Refine ran on, (n_hyp+1) entries each of which n_records are live: first the state's best_inlier set when best_inliers > 0 (rec_hyp = -1), then each
     * record up to the hypothesis that ended the call (records past it leave no trace; entries past n_records are zero) */
    int32_t* rec_hyp;           /* position of the record in the chunk, -1 for the carried set */
    double* rec_R;              /* *9: mRi of Refine's compute_pose */
    double* rec_t;              /* *3 */
    int32_t* rec_inliers;       /* mnRefinedInliers; Refine succeeded when it is > min_inliers */
    uint8_t* rec_inlier;        /* *n: mvbRefinedInliers */
} eao_pnp_solver_result;

/* PnPsolver::iterate with mRansacMinInliers = min_inliers, mRansacMaxIts = max_its (the values SetRansacParameters :121-157 leaves; the adapter computes them)
 * and mRansacMinSet = min_set (4 .. 64).  sets: n_hyp*min_set indices into 0 .. n-1 in draw order; an index may repeat inside a set (the sampling loop of
 * :191-201 can produce that).  n_hyp is the number of passes the loop `while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)` (:182) makes: note
 * the ||, it is max(nIterations, max_its - iterations), so the first iterate(5) of Relocalization runs all of its max_its.  All n_hyp hypotheses are evaluated.
 * In order: a hypothesis with inliers >= min_inliers and inliers > best_inliers (strict) is a record and becomes the best; at every hypothesis that passes the
 * >= gate upstream runs Refine on the best set, which is deterministic, so it is computed once per record (and once for the set the state carries in); the first
 * gate-passing hypothesis whose best set refines to more than min_inliers (strict) inliers ends the call: iterations advances up to and including it.  Otherwise
 * no_more = iterations >= max_its, and with it the best pose returns when best_inliers >= min_inliers.  n < min_inliers: no_more, nothing evaluated, state untouched.
 * EAO_ERR_INVALID before anything is written: an index out of range, min_set < 4 or > 64, a non-finite input, n < min_set, a best_inlier set whose size is not
 * best_inliers.
 * Arithmetic: EPnP in double, op for op (-ffp-contract=off); CheckInliers with upstream's mixed widths.  OpenCV's parts: cvSVD of the symmetric 3 x 3 and 12 x 12
 * is a cyclic Jacobi eigen-solve in double with a fixed sweep count, singular values |lambda| descending (the lower index first among equals); the 3 x 3 SVD of ABt
 * by the scheme of the Initializer's (eigenvectors of A^T A, u = A v normalised); cvInvert / cvSolve(CV_SVD) are the minimum-norm least-squares solution through
 * a one-sided Jacobi SVD, a singular value counting when it exceeds 2 * DBL_EPSILON * (the sum of all of them).  Two deviations from upstream:
 *  1. The PCA axes of choose_control_points (the rows of UCt) are signed so that the component of largest magnitude is positive (the lowest index wins a tie);
 *     upstream's sign is cvSVD's, and the pose depends on it at the noise level.
 *  2. gauss_newton's X starts at zero; upstream's is uninitialised when qr_solve leaves through its `eta == 0` return in the first iteration.
 * Nothing is repaired: coplanar or repeated points, a zero depth and a NaN flow through; a NaN error2 is an outlier.  With min_set = 4 the null space of M^T M has
 * four dimensions and a hypothesis' pose depends on the basis the eigen-solver returns: it is this library's, not upstream's.  Two calls on the same arguments
 * return the same bytes. */
eao_status eao_pnp_solver_iterate(const eao_pnp_solver_problem* problem, int32_t min_inliers, int32_t max_its, int32_t min_set, eao_pnp_solver_state* state,
                                  const int32_t* sets, int32_t n_hyp, eao_pnp_solver_result* result);

/* One round of Relocalization's loop over its candidates (src/Tracking.cc:2847-2870) in one launch chain: problem b with min_inliers[b], max_its[b], min_set[b],
 * states[b], sets[b] (n_hyp[b]*min_set[b] indices) and results[b].  Each result and state is bit-identical to what eao_pnp_solver_iterate returns for it.  Any
 * invalid problem fails the call before anything is written. */
eao_status eao_pnp_solver_iterate_batch(int32_t n_problems, const eao_pnp_solver_problem* problems, const int32_t* min_inliers, const int32_t* max_its,
                                        const int32_t* min_set, eao_pnp_solver_state* states, const int32_t* const* sets, const int32_t* n_hyp,
                                        eao_pnp_solver_result* results);

/* Diagnostic (tools/bench_pnp_solver.py): with EAO_PNP_EVENTS=1 in the environment, the device time in ms of each of the four kernels of this thread's last
 * eao_pnp_solver_iterate / _batch (hypotheses, scan, refine, finish), from HIP events on its stream.  An event call that fails costs that measurement
 * (-1 in its slot) and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_pnp_solver_last_kernel_ms(float* kernel_ms /* 4 */);

/* ------------------------------------------------------------------------------------------------
 * ORBVocabulary (reference include/ORBVocabulary.h = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h):
 * the vocabulary tree on the device.  Frame::ComputeBoW (src/Frame.cc:764-771, called at src/Tracking.cc:1571 and :2789), KeyFrame::ComputeBoW
 * (src/KeyFrame.cc:93-101, called at src/LocalMapping.cc:141 and src/Tracking.cc:1424-1425) and ORBVocabulary::score (src/LoopClosing.cc:134,
 * src/KeyFrameDatabase.cc:132, 248) stand behind these entry points.  Everything is bit for bit what upstream computes, the doubles included: every double is
 * the result of single IEEE operations in upstream's order.
 *
 * The handle.  The five arrays are what both upstream file formats hold per node (TemplatedVocabulary.h:1350-1480); array entry i is node id i + 1 in file
 * order, the root (id 0) is implied.  The children of a node are its nodes in ascending id (the loaders' push_back order, the order ties are broken in); word ids
 * count the leaf-flagged nodes in id order (:1420-1427, :1468-1473).  The descent stops at a node without children (:1266, :340), so eao_vocabulary_create
 * fails with EAO_ERR_INVALID -- before anything reaches the device -- when is_leaf[i] disagrees with "no node names i + 1 as its parent", when parent[i] is not in
 * 0 .. i, or on an enum out of range.  n_nodes == 0 is a valid, empty vocabulary (empty(), :1146): every transform over it returns empty vectors and zeroed
 * feat_* arrays.  depth (upstream's m_L) is DERIVED: the largest depth of a leaf (a child of the root has depth 1); a file whose header names another L than its
 * tree has differs from upstream in the node ids of the FeatureVector only.  The arrays are copied; the handle is immutable and any number of host threads may
 * use it at once (each thread has its own stream and scratch).  On the device the children of one node are contiguous; file ids and word ids are what is
 * reported outward. */
typedef struct eao_vocabulary eao_vocabulary;
typedef struct {
    int32_t n_nodes;            /* nodes WITHOUT the root; array entry i is node id i+1, in file order */
    const int32_t* parent;      /* parent id, 0 = root; required: 0 <= parent[i] < i+1 */
    const uint8_t* descriptor;  /* n_nodes*32 */
    const double*  weight;      /* Node::weight (WordValue is double; the binary file stores float, promoted) */
    const uint8_t* is_leaf;     /* the file's leaf flag */
    int32_t weighting;          /* DBoW2 enum order: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY */
    int32_t norm;               /* what mustNormalize() yields: 0 none, 1 L1, 2 L2 */
} eao_vocabulary_desc;
eao_status eao_vocabulary_create(const eao_vocabulary_desc* desc, eao_vocabulary** out);
void eao_vocabulary_destroy(eao_vocabulary* voc);
/* each pointer may be NULL; n_words = size(), depth and max_children as defined above (0 for the empty vocabulary) */
eao_status eao_vocabulary_info(const eao_vocabulary* voc, int32_t* n_nodes, int32_t* n_words, int32_t* depth, int32_t* max_children);

/* TemplatedVocabulary::transform(features, v, fv, levelsup), :1138-1206, with the per-feature descent of :1229-1271.
 * Descent: from the root, each level takes the child with the smallest FORB::distance (FORB.cpp:81-101); strict <, so the first child in id order wins a tie;
 * until a node without children.  nid is the node reached at level depth - levelsup (the first chosen child is level 1); a level <= 0 gives nid = 0.  A leaf
 * reached ABOVE that level leaves nid uninitialised upstream (:1163, :1263); here nid is then the leaf's own node id and feat_stopped bit 1 is set.
 * A feature whose word weight is not > 0 enters neither vector (:1169, :1197; feat_stopped bit 0).  TF_IDF / TF: addWeight adds the weight once per feature in
 * feature order (BowVector.cpp:34-46: c - 1 sequential additions for a word seen c times), and without normalisation every value is divided by v.size()
 * (:1176-1182).  IDF / BINARY: addIfNotExist, the weight once.  Normalisation (BowVector.cpp:62-84): L1 the sequential sum of fabs(value) in ascending word id,
 * L2 the sequential sum of squares, then sqrt; each value divided when the norm is > 0.  FeatureVector (FeatureVector.cpp:31-45): node ids ascend, each node's
 * indices ascend.  n <= EAO_VOCABULARY_MAX_FEATURES per frame; more fails with EAO_ERR_INVALID and nothing is written.  levelsup >= 0.
 * The result arrays are the caller's: capacities n (word_id, word_value, node_id, index, feat_*) and n + 1 (node_start); entries past the counts are not
 * written.  EAO_ERR_INVALID leaves every output untouched.  Two calls on the same arguments return the same bytes. */
#define EAO_VOCABULARY_MAX_FEATURES 8192
typedef struct {
    int32_t n_words;   uint32_t* word_id;  double* word_value;                  /* BowVector in std::map order; capacity n */
    int32_t n_fv_nodes; uint32_t* node_id; int32_t* node_start; uint32_t* index; /* FeatureVector, the layout of eao_feature_vector; capacities n, n+1, n */
    uint32_t* feat_word; uint32_t* feat_node; uint8_t* feat_stopped;            /* optional (NULL): per feature, for inspection */
} eao_bow_result;
eao_status eao_vocabulary_transform(const eao_vocabulary* voc, const uint8_t* desc, int32_t n, int32_t levelsup, eao_bow_result* result);
/* n_frames frames in one upload, one launch chain and one copy back: frame f owns descriptors frame_start[f] .. frame_start[f+1] - 1 (frame_start[0] = 0,
 * ascending) and results[f]; equal to n_frames single calls entry for entry. */
eao_status eao_vocabulary_transform_batch(const eao_vocabulary* voc, int32_t n_frames, const uint8_t* desc, const int32_t* frame_start /* n_frames+1 */,
                                          int32_t levelsup, eao_bow_result* results);
/* The same over the descriptors and the count ONE frame's slice of eao_orb_extract_batch_device left in HBM (d_desc: cap*32 bytes, 16-byte aligned; d_n: that
 * frame's count, read on the device).  Enqueued on `stream` (a hipStream_t; NULL = the null stream) behind whatever wrote them, and waited for: the result
 * arrays are host arrays of capacity cap (cap + 1).  A count outside 0 .. cap fails with EAO_ERR_INVALID after the chain, outputs untouched.  This is the hook for
 * keeping TrackReferenceKeyFrame's chain on the device; eao_tracker_track_reference_keyframe itself still takes fv_cur. */
eao_status eao_vocabulary_transform_device(const eao_vocabulary* voc, const uint8_t* d_desc, const int32_t* d_n, int32_t cap, int32_t levelsup,
                                           eao_bow_result* result, void* stream);

/* L1Scoring::score (ScoringObject.cpp:23-68) of ONE query vector (v1: q_id / q_val, nq entries) against n_db stored vectors (v2: vector j owns entries
 * db_start[j] .. db_start[j+1] - 1 of db_id / db_val) -- the loops of src/KeyFrameDatabase.cc:124-138, 243-254 and src/LoopClosing.cc:125-138 in one call.
 * Per pair, over the common word ids in ascending order: s += fabs(vi - wi) - fabs(vi) - fabs(wi), evaluated left to right and accumulated sequentially from 0;
 * scores[j] = -s / 2.0 (no common word: -0.0, as upstream).  Ids ascend strictly within each vector and db_start ascends from >= 0, else EAO_ERR_INVALID before
 * anything is written.  Callers narrow to float themselves, as upstream does. */
eao_status eao_bow_score_l1(int32_t nq, const uint32_t* q_id, const double* q_val, int32_t n_db, const int32_t* db_start /* n_db+1 */, const uint32_t* db_id,
                            const double* db_val, double* scores /* n_db */);

/* ------------------------------------------------------------------------------------------------
 * KeyFrameDatabase (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc): the recognition database at the head of LoopClosing::DetectLoop
 * (src/LoopClosing.cc:141) and Tracking::Relocalization.  The BoW vectors of the added keyframes are RESIDENT on the device (one arena of word ids, one of
 * values); a query uploads the query vector and downloads 16 bytes per live keyframe.  No inverted file is kept: upstream's walk over mvInvertedFile is, per
 * stored keyframe, the number of the query's words it holds, and the list order of lKFsSharingWords is ascending (first common word, add order)
 * (csrc/keyframe_db_internal.h says why).  Everything is bit for bit what upstream computes: counts, list orders, the float scores, the candidates.
 *
 * Per-keyframe state.  Upstream keeps mnLoopQuery / mnLoopWords / mLoopScore and mnRelocQuery / mnRelocWords / mRelocScore on the KeyFrame
 * (include/KeyFrame.h:207-212); the handle keeps the same six per held id, initial state (0, 0, unset) as src/KeyFrame.cc:37 leaves them.  An id the handle does
 * not hold (never added, or erased) reads as the initial state.  A score that was never written reads as 0.0f where upstream reads an uninitialised float, and
 * stage 2 counts such reads (used_unset).
 * Deviations: adding an id that is live is EAO_ERR_INVALID (upstream would list it twice); erasing an unknown id is a no-op, as upstream; a re-added id starts with
 * fresh state; word ids at or above n_words are EAO_ERR_INVALID (upstream indexes past the vector).  A vector, stored or query, has at most
 * EAO_VOCABULARY_MAX_FEATURES words.
 * EAO_ERR_INVALID leaves every output and all state untouched.  A handle is serialised by one mutex (upstream's mMutex, widened to the whole call); distinct
 * handles are independent.  The arenas grow by reallocation (device-to-device copy), and the words of erased keyframes are compacted away once they exceed half
 * of the words in use. */
typedef struct eao_keyframe_db eao_keyframe_db;
/* KeyFrameDatabase::KeyFrameDatabase (:33-37): n_words = voc.size() */
eao_status eao_keyframe_db_create(int32_t n_words, eao_keyframe_db** out);
void eao_keyframe_db_destroy(eao_keyframe_db* db);
/* clear() (:68-72): drops every keyframe and its state */
eao_status eao_keyframe_db_clear(eao_keyframe_db* db);
/* each pointer may be NULL: live keyframes, the words in use in the arena (those of erased keyframes included until they are compacted away), the arena's
 * capacity in words */
eao_status eao_keyframe_db_info(eao_keyframe_db* db, int32_t* n_live, int64_t* n_stored_words, int64_t* arena_capacity);
/* add(pKF) (:39-45): pKF->mnId and pKF->mBowVec in std::map order.  Ids ascend strictly, else EAO_ERR_INVALID.  n == 0 is valid; such a keyframe is never listed. */
eao_status eao_keyframe_db_add(eao_keyframe_db* db, uint64_t kf_id, int32_t n, const uint32_t* word_id, const double* word_val);
/* erase(pKF) (:47-66) */
eao_status eao_keyframe_db_erase(eao_keyframe_db* db, uint64_t kf_id);
/* The kernel's raw result over the *n_live live keyframes in storage (= add) order: the number of common words (what the walks of :85-103 / :206-221 count), the
 * smallest common word id (unspecified where common == 0) and the double of L1Scoring::score(query, stored) exactly as eao_bow_score_l1 gives it (-0.0 without a
 * common word).  Pure: no per-keyframe state is touched, two calls return the same bytes.  It also gives src/LoopClosing.cc:125-138 its scores for the connected
 * keyframes that are resident.  cap: the capacity of the four arrays; below the number of live keyframes is EAO_ERR_INVALID. */
eao_status eao_keyframe_db_intersect(eao_keyframe_db* db, int32_t nq, const uint32_t* q_id, const double* q_val, int32_t cap, uint64_t* kf_id, int32_t* common,
                                     uint32_t* first_word, double* score, int32_t* n_live);
/* Stage 1: DetectLoopCandidates :75-141 (kind 0) / DetectRelocalizationCandidates :198-255 (kind 1) up to lScoreAndMatch; writes the per-keyframe state as upstream
 * does.  kind 0: connected_id = the ids of pKF->GetConnectedKeyFrames() in any order (ids not held are ignored) and min_score; kind 1 reads neither. */
typedef struct {
    int32_t kind;                  /* 0 DetectLoopCandidates, 1 DetectRelocalizationCandidates */
    uint64_t query_id;             /* pKF->mnId / F->mnId */
    int32_t nq; const uint32_t* q_id; const double* q_val;     /* mBowVec in std::map order */
    int32_t n_connected; const uint64_t* connected_id;
    float min_score;
} eao_keyframe_db_query;
typedef struct {
    int32_t n_sharing; uint64_t* sharing_id; int32_t* sharing_words;   /* lKFsSharingWords in list order with mnLoopWords / mnRelocWords; capacity cap */
    int32_t max_common_words, min_common_words, n_scores;             /* :112-121, :227-238; all 0 when the list is empty */
    int32_t n_scored; uint64_t* scored_id; float* scored_score;       /* lScoreAndMatch in list order; capacity cap */
} eao_keyframe_db_scored;
eao_status eao_keyframe_db_query_scores(eao_keyframe_db* db, const eao_keyframe_db_query* query, int32_t cap, eao_keyframe_db_scored* out);
/* Stage 2, host only: :143-195 (kind 0) / :257-307 (kind 1).  nb_start / nb_id: GetBestCovisibilityKeyFrames(10) of every scored keyframe as a CSR; the
 * neighbours' state is read from the handle.  cand_id (capacity n_scored): vpLoopCandidates / vpRelocCandidates in upstream's order.  acc_score / best_id
 * (n_scored each, optional): lAccScoreAndMatch.  kind 1 ignores min_common_words and min_score, as upstream. */
eao_status eao_keyframe_db_candidates(eao_keyframe_db* db, int32_t kind, uint64_t query_id, int32_t min_common_words, float min_score, int32_t n_scored,
                                      const uint64_t* scored_id, const float* scored_score, const int32_t* nb_start /* n_scored+1 */, const uint64_t* nb_id,
                                      uint64_t* cand_id, int32_t* n_cand, float* acc_score, uint64_t* best_id, int32_t* used_unset);

/* ------------------------------------------------------------------------------------------------
 * MapPlane boundaries (reference include/MapPlane.h, src/MapPlane.cc; Map::AssociatePlanesByBoundary src/Map.cc:155-215, Map::PointDistanceFromPlane :217-236,
 * Map::SearchMatchedPlanes :245-292): the plane association that runs in front of Optimizer::PoseOptimization in all three tracking stages
 * (src/Tracking.cc:1587, :2181, :2243, :2491) and in LoopClosing (src/LoopClosing.cc:395, :620).  The boundary clouds of the map's planes
 * (MapPlane::mvBoundaryPoints, world frame) are RESIDENT on the device, 16 bytes per point; a query uploads the frame's plane coefficients and 32 bytes per
 * candidate, and downloads one index and one distance per frame plane.  Everything is bit for bit what upstream's loops compute.
 *
 * The handle keeps, per plane id, the cloud and mWorldPos.  The table is in ADD order; update_boundary does not move a plane in it.
 * Deviations: adding an id that is live is EAO_ERR_INVALID (upstream's ids are unique, src/MapPlane.cc:26); erasing an unknown id is a no-op, as
 * std::set::erase (src/Map.cc:150); a candidate id the handle does not hold is EAO_ERR_INVALID.
 * EAO_ERR_INVALID leaves every output and all state untouched.  A handle is serialised by one mutex (upstream's mMutexMap, widened to every call); distinct
 * handles are independent.  The arena grows by reallocation (device-to-device copy), and replaced and erased clouds are compacted away once they exceed half of
 * the points in use. */
#define EAO_PLANE_MAP_MAX_ROWS 2048          /* frame planes (rows of coef) per eao_plane_map_associate call */
#define EAO_PLANE_MAP_MAX_POINTS 1048576     /* points of one plane's cloud */
#define EAO_PLANE_MAP_MAX_CANDIDATES 65536   /* candidates per call; rows x candidates <= 2^24 */
#define EAO_PLANE_MAP_DIS_TH 0.2f            /* Map::mfDisTh, src/Map.cc:22 */
#define EAO_PLANE_MAP_ANGLE_TH 0.8f          /* Map::mfAngleTh, src/Map.cc:23 */
typedef struct eao_plane_map eao_plane_map;
eao_status eao_plane_map_create(eao_plane_map** out);
void eao_plane_map_destroy(eao_plane_map* pm);
/* Map::clear (src/Map.cc:131-133): drops every plane; the allocation stays */
eao_status eao_plane_map_clear(eao_plane_map* pm);
/* each pointer may be NULL: live planes, the points in use in the arena (those of replaced and erased clouds included until they are compacted away), the
 * arena's capacity in points */
eao_status eao_plane_map_info(eao_plane_map* pm, int32_t* n_live, int64_t* n_points_in_use, int64_t* arena_capacity);
/* MapPlane::MapPlane (src/MapPlane.cc:23-39): world_pos = Pos (4 floats), xyz = pRefKF->mvBoundaryPoints[idx] as n x 3 floats in the camera frame, Tcw =
 * pRefKF->GetPose() as 16 floats, row-major.  The cloud is stored as pcl::transformPointCloud(cloud, out, T.inverse().matrix()) with Eigen::Isometry3d T =
 * Converter::toSE3Quat(Tcw) leaves it (:34-36): the isometry in double (unit quaternion of the rotation block, then its rotation matrix), inverted as
 * R^T, -(R^T t), and per coordinate (float)(m0*x + m1*y + m2*z + m3) in double, left to right.  Non-finite coordinates go through the same arithmetic.
 * Tcw == NULL: the points are in the world frame already and are stored as they are.  n == 0 is valid.  A live id is EAO_ERR_INVALID. */
eao_status eao_plane_map_add(eao_plane_map* pm, uint64_t id, const float* world_pos /* 4 */, int32_t n, const float* xyz /* n*3 */, const float* Tcw /* 16 or NULL */);
/* MapPlane::UpdateBoundary (src/MapPlane.cc:150-153; called at src/Tracking.cc:1112): replaces the plane's cloud, same transform.  An id that is not held is
 * EAO_ERR_INVALID. */
eao_status eao_plane_map_update_boundary(eao_plane_map* pm, uint64_t id, int32_t n, const float* xyz, const float* Tcw);
/* MapPlane::SetWorldPos (src/MapPlane.cc:137-142), also for what the optimisers write back.  An id that is not held is EAO_ERR_INVALID. */
eao_status eao_plane_map_set_world_pos(eao_plane_map* pm, uint64_t id, const float* world_pos /* 4 */);
/* Map::EraseMapPlane (src/Map.cc:147-153) and the losing side of MapPlane::Replace (src/MapPlane.cc:161-192).  An unknown id is a no-op. */
eao_status eao_plane_map_erase(eao_plane_map* pm, uint64_t id);
/* The resident world-frame cloud of a plane (*n points into xyz, capacity cap points; cap below the count is EAO_ERR_INVALID) and, when world_pos is not NULL, its
 * mWorldPos.  xyz == NULL: the count (and world_pos) alone. */
eao_status eao_plane_map_boundary(eao_plane_map* pm, uint64_t id, int32_t cap, float* xyz /* cap*3 */, int32_t* n, float* world_pos /* 4 or NULL */);
/* Map::AssociatePlanesByBoundary (src/Map.cc:155-215; M = mTcw) and Map::SearchMatchedPlanes (:245-292; M = Scw) for n_sets frames against ONE candidate list
 * (n_sets > 1: the connected keyframes of LoopClosing::SearchAndFuse, src/LoopClosing.cc:620).  Set s owns M + 16*s (row-major 4x4) and rows set_start[s] ..
 * set_start[s+1] - 1 of coef (mvPlaneCoefficients, 4 floats per row, camera frame); set_start[0] = 0, ascending.  cand_id: the candidates in the caller's
 * iteration order -- std::set order of Map::mspMapPlanes, vector order of vpPlanes; an id may appear twice.  cand_id == NULL: every live plane in add order, and
 * n_cand must be their number (or 0: no candidates).
 * Per row: pM = M^T c as a cv::Mat product (accumulated in double, rounded once to float; src/Frame.cc:373-379).  Per candidate in list order: angle = pM0*pW0 +
 * pM1*pW1 + pM2*pW2 in float, left to right; the pair is gated in when angle > angle_th || angle < -angle_th (a NaN is not).  For a gated pair dis starts at
 * 100 and takes d = |pM0*x + pM1*y + pM2*z + pM3| (float, left to right) of every point with d < dis (a NaN never wins; no points leave 100).  ldTh starts at
 * dis_th; a gated candidate with dis < ldTh becomes the match and sets ldTh = dis: the first of equal minima wins, a distance equal to dis_th does not associate.
 * match (rows): the index into the candidate list or -1; match_dis (rows): ldTh as the loop leaves it (dis_th where nothing associated).  Optional (NULL):
 * world_coef (rows x 4) = pM; dis (rows x n_cand, row-major) with 100 where the pair is gated out; gated (rows x n_cand).
 * No rows or no candidates are valid calls.  Two calls on the same arguments return the same bytes. */
eao_status eao_plane_map_associate(eao_plane_map* pm, int32_t n_sets, const float* M /* n_sets*16 */, const int32_t* set_start /* n_sets+1 */,
                                   const float* coef /* rows*4 */, int32_t n_cand, const uint64_t* cand_id, float dis_th, float angle_th, int32_t* match,
                                   float* match_dis, float* world_coef, float* dis, uint8_t* gated);

/* ---- Plane segmentation: Frame::ComputePlanesFromPEAC (src/Frame.cc:381-460), called from the RGB-D constructor (:240) --------------------------------------
 * The depth image becomes the organised cloud of src/Frame.cc:391-405, PEAC segments it (include/PEAC/AHCPlaneFitter.hpp run :209-258: initGraph :784-953,
 * ahCluster :981-1187, refineDetails :297-377 with findBlockMembership :483-585 and floodFill :426-474, at the constructor defaults of :152-156: doRefine,
 * ERODE_ALL_BORDER, INIT_STRICT; nothing else is offered), and every plane's points go through pcl::VoxelGrid (src/Frame.cc:435-439) and PlaneNotSeen
 * (:349-371).  The two passes over all pixels run on the device, the block graph between them on the host (csrc/plane_seg_internal.h); the readings this
 * build fixes where upstream leaves a value or an order open are in DESIGN.md section 4k.  The ParamSet is in millimetre units although the cloud is in
 * metres: upstream's behaviour, kept.
 * A handle is serialised by one mutex; distinct handles run side by side on the Latency stream class.  An invalid ARGUMENT (a NULL, a stride below the width, a
 * capacity below the count, an index out of range) leaves every output and all state untouched.  Two EAO_ERR_INVALID returns of eao_plane_seg_run depend on the
 * image instead and come after the run has started: more than EAO_PLANE_SEG_MAX_PLANES final planes, and a voxel grid past INT_MAX cells for one plane or
 * EAO_PLANE_SEG_MAX_CELLS for all.  These two, like a device error, DROP THE PREVIOUS FRAME'S RESULTS: the handle is left without results and the read-backs
 * fail with EAO_ERR_INVALID until the next successful run.  Two runs on the same image return the same bytes, on one handle or on two. */
#define EAO_PLANE_SEG_MAX_PIXELS (1 << 22)       /* width * height */
#define EAO_PLANE_SEG_MAX_WINDOW 32              /* window: 2 .. 32 */
#define EAO_PLANE_SEG_MAX_PLANES 64              /* final planes of one frame; more is EAO_ERR_INVALID from eao_plane_seg_run */
#define EAO_PLANE_SEG_MAX_CELLS 0x7fffffff       /* voxel cells of all final planes' grids together; one plane's grid past INT_MAX is refused as PCL refuses it */
typedef struct {
    int32_t width, height;
    float fx, fy, cx, cy;              /* the Frame's static floats (src/Frame.cc:401-402) */
    int32_t window;                    /* windowWidth == windowHeight (AHCPlaneFitter.hpp:154) */
    int32_t min_support, max_step;     /* :153 */
    float leaf;                        /* src/Frame.cc:436 */
    double depth_min, depth_max;       /* src/Frame.cc:396: a pixel is invalid if isnan(d) || d > depth_max || d < depth_min */
    /* ParamSet, AHCParamSet.hpp:68-76 */
    double depth_sigma, std_tol_init, std_tol_merge;
    double z_near, z_far, angle_near, angle_far;
    double similarity_merge, similarity_refine;
    double depth_alpha, depth_change_tol;
} eao_plane_seg_cfg;
/* One window x window block after the block constructor (AHCPlaneSeg.hpp:211-285) and Stats::compute (:125-156).  flag: bit 0 the block holds an invalid pixel,
 * bit 1 a valid pixel of it differs from a valid right / lower neighbour by more than T_dz; 0: N = window * window and the rest is filled.  A flagged block has
 * N = 0, zero sums, centre and normal, and the quiet NaN 0x7ff8000000000000 as mse and curvature. */
typedef struct {
    int32_t flag, N;
    double sums[9];                    /* sx sy sz sxx syy szz sxy syz sxz, each accumulated in row-major order */
    double center[3], normal[3], mse, curvature;
} eao_plane_seg_block;
/* One entry of plane_filter.extractedPlanes after run() (src/Frame.cc:425-456), in its order.  coef: (nx, ny, nz, d) as floats, negated when d < 0 (:441-445);
 * kept: PlaneNotSeen against the kept planes before it (:447); cloud_offset / cloud_count: its voxel centroids among the handle's points (16 bytes each on the
 * device); n_pixels: plane_vertices_[i].size(). */
typedef struct {
    double normal[3], center[3], mse, curvature;
    int32_t N, rid;
    float coef[4];
    int32_t kept, cloud_offset, cloud_count, n_pixels;
} eao_plane_seg_plane;
typedef struct eao_plane_seg eao_plane_seg;
/* PlaneFitter() (AHCPlaneFitter.hpp:152-156), ParamSet() (AHCParamSet.hpp:68-76) and the literals of src/Frame.cc:396 and :436 */
void eao_plane_seg_cfg_default(eao_plane_seg_cfg* cfg, int32_t width, int32_t height, float fx, float fy, float cx, float cy);
eao_status eao_plane_seg_create(const eao_plane_seg_cfg* cfg, eao_plane_seg** out);
void eao_plane_seg_destroy(eao_plane_seg* h);
/* Frame::ComputePlanesFromPEAC(imDepth) (src/Frame.cc:381-460): depth is height rows of width floats, `stride` floats apart (>= width).  The results stay in
 * the handle until the next run. */
eao_status eao_plane_seg_run(eao_plane_seg* h, const float* depth, int32_t stride);
/* Counts of the last run: planes (plane_num_, :410), points of all clouds, blocks, pixels the flood fill claimed.  Any pointer may be NULL. */
eao_status eao_plane_seg_info(eao_plane_seg* h, int32_t* n_planes, int32_t* n_points, int32_t* n_blocks, int32_t* n_claims);
/* The plane table (:425-456).  planes == NULL: only *n.  cap below the count is EAO_ERR_INVALID. */
eao_status eao_plane_seg_planes(eao_plane_seg* h, int32_t cap, eao_plane_seg_plane* planes, int32_t* n);
/* coarseCloud of plane `plane` (:435-439, the public PCL 1.8 VoxelGrid: one centroid per occupied voxel in ascending voxel index, each the float sum of its
 * points in ascending pixel index over the float count), whether kept or not.  xyz == NULL: only *n. */
eao_status eao_plane_seg_cloud(eao_plane_seg* h, int32_t plane, int32_t cap, float* xyz /* cap*3 */, int32_t* n);
/* membershipImg after refineDetails (AHCPlaneFitter.hpp:358-370) as width * height plane indices, -1 where upstream paints black */
eao_status eao_plane_seg_membership(eao_plane_seg* h, int32_t* image /* width*height */);
/* The per-block records of the last run, (height / window) * (width / window) of them in row-major block order; for the tests.  blocks == NULL: only *n. */
eao_status eao_plane_seg_blocks(eao_plane_seg* h, int32_t cap, eao_plane_seg_block* blocks, int32_t* n);
/* What the host's middle handed to the device, for the tests: blkMap (:131, one per block, indices into the planes of the FIRST ahCluster), plidmap (:327-342)
 * and the pixels floodFill claimed as (pixel, plane) pairs in ascending pixel order.  Any array may be NULL. */
eao_status eao_plane_seg_middle(eao_plane_seg* h, int32_t* blk_map, int32_t cap_old, int32_t* plidmap, int32_t* n_old, int32_t cap_claims, int32_t* claims /* cap_claims*2 */,
                                int32_t* n_claims);
/* Per-stage times of eao_plane_seg_run, for tools/bench_plane_segmentation.py.  With profiling on a run waits once more (behind the upload), so that the stages
 * can be told apart; results are unchanged.  us[4], microseconds on the host's clock, every stage ending in a wait: upload of the depth image; k_ps_block_init
 * and the download of the block records; the host's middle; membership and the voxel stage.  EAO_ERR_INVALID when the last run did not have profiling on. */
eao_status eao_plane_seg_set_profiling(eao_plane_seg* h, int32_t on);
eao_status eao_plane_seg_last_timing(eao_plane_seg* h, double* us /* 4 */);
/* eao_plane_map_add / eao_plane_map_update_boundary (MapPlane::MapPlane, src/MapPlane.cc:34-37; UpdateBoundary, :150-153) with the cloud taken from the kept
 * plane `plane` (an index into eao_plane_seg_planes) of a segmentation handle's last run, device to device: mvBoundaryPoints[i] of the frame never visits the
 * host.  The same transform kernel and the same table as the host-pointer forms: the resident bytes are those of eao_plane_map_add on the read-back cloud.  A plane
 * that was not kept, an index out of range and a handle without results are EAO_ERR_INVALID; nothing changes then.  The map's mutex is taken first, then the
 * segmentation handle's. */
eao_status eao_plane_map_add_from_seg(eao_plane_map* pm, uint64_t id, const float* world_pos /* 4 */, eao_plane_seg* seg, int32_t plane, const float* Tcw /* 16 or NULL */);
eao_status eao_plane_map_update_boundary_from_seg(eao_plane_map* pm, uint64_t id, eao_plane_seg* seg, int32_t plane, const float* Tcw /* 16 or NULL */);

/* ---- Object layer: Object_Map::IsolationForestDeleteOutliers (src/Object.cc:1239-1348; called at :718, :1596, :1692, :1699) ---------------------------------
 * The isolation forest of include/isolation_forest.h over an object's map points: IsolationForest::Build (:448-477), IsolationTree::Build (:301-345), Node::Build
 * (:165-224), GetAnomalyScores (:499-529).  Every forest is a pure function of its point list, and the result is bit for bit what the reference's header
 * computes under libstdc++ (g++ 11): std::mt19937, std::shuffle's two-swaps-per-draw path, uniform_int_distribution's multiply-and-reject method,
 * generate_canonical<float, 24> and u * (b - a) + a rounded operation by operation (csrc/iforest_internal.h).  One wavefront builds one
 * tree; one wavefront scores one point, a lane per tree; the host divides by the tree count and applies libm's pow.
 * The entries are stateless; each host thread has its own stream and staging.  EAO_ERR_INVALID leaves every output untouched.  Two calls on the same arguments
 * return the same bytes, on one thread or on several.
 *
 * eao_iforest_scores_batch: the general entry.  Object j owns points start[j] .. start[j+1] - 1 of xyz (3 floats each; start[0] >= 0, ascending) and entry j of
 * tree_count, seed and sample_size (Build's treeCount, seed, sampleSize).  scores and total_path_len (optional) are indexed like the points: per point the
 * score pow(2, -(total / tree_count) / C(sample_size)) (:524-526; NaN where C is 0, as upstream) and the total path length over the trees in index order
 * (:517-522).  stream_start (optional, n_obj + 1 entries) receives the byte offsets of the objects' streams; stream (optional, needs stream_start; capacity
 * stream_cap bytes) the exact bytes of IsolationForest::Serialize (:532-560) per object, back to back: a 16-byte forest header (size_t 3, tree count, sample
 * size), per tree a 12-byte header (size_t 3, sample size) and the 12-byte node records {dim u32, split f32, size u32} in preorder, size == 0 on inner nodes.
 * A stream buffer that is too short is EAO_ERR_CAPACITY: stream_start is filled, nothing else is written.
 * Refused with EAO_ERR_INVALID: sample_size == 0, sample_size above the object's points, tree_count == 0, a non-finite coordinate (it breaks std::sort's
 * ordering contract upstream: undefined behaviour), more than EAO_IFOREST_MAX_POINTS points (libstdc++'s shuffle takes its other path above), and an object on
 * which upstream's own Build returns false (a split rounded above the maximum of its range, :167). */
#define EAO_IFOREST_MAX_POINTS 65535
#define EAO_OBJECT_IFOREST_TREES 50             /* src/Object.cc:1296 */
#define EAO_OBJECT_IFOREST_SEED 12345           /* :1296 */
#define EAO_OBJECT_IFOREST_MIN_POINTS 30        /* :1256 */
#define EAO_OBJECT_IFOREST_EXEMPT_CLASS_A 75    /* :1245 */
#define EAO_OBJECT_IFOREST_EXEMPT_CLASS_B 64
#define EAO_OBJECT_IFOREST_EXEMPT_CLASS_C 65
eao_status eao_iforest_scores_batch(int32_t n_obj, const int32_t* start /* n_obj+1 */, const float* xyz, const int32_t* tree_count /* n_obj */,
                                    const uint32_t* seed /* n_obj */, const int32_t* sample_size /* n_obj */, double* scores, double* total_path_len,
                                    uint8_t* stream, int64_t stream_cap, int64_t* stream_start /* n_obj+1 */);
/* The whole of Object_Map::IsolationForestDeleteOutliers for a batch of objects: xyz = GetWorldPos() of mvpMapObjectMappoints in vector order, class_id =
 * mnClass, bi_forest = the file-level flag biForest (:1241).  An object runs when bi_forest is set, its class is none of 75 / 64 / 65 (:1245) and it has at least
 * 30 points (:1256); then Build(50, 12345, data, N / 2) (:1296) and a point is flagged when its score exceeds th = 0.6f, or 0.65f for class 62 (:1248-1250,
 * :1317; th is a float promoted to double).  flags (one byte per point, indexed like the points): 1 = erase; removed (n_obj): the number flagged; scores
 * (optional): the anomaly scores, -1.0 for the points of objects the rules skip.  Skipped objects come back without flags and cost no device work, and their
 * points are not read.  An object on which upstream's Build returns false comes back without flags, as upstream leaves it.  A non-finite coordinate in an
 * object that runs is EAO_ERR_INVALID for the whole call.  The caller erases exactly the flagged indices (upstream's own loop reads outliernum one past its
 * end after the last outlier, :1336; include/eaofusion/ObjectMap.h does not). */
eao_status eao_object_iforest_outliers_batch(int32_t n_obj, const int32_t* start /* n_obj+1 */, const float* xyz, const int32_t* class_id /* n_obj */,
                                             int32_t bi_forest, uint8_t* flags, int32_t* removed /* n_obj */, double* scores);
/* Diagnostic (tools/bench_isolation_forest.py): after eao_iforest_set_profiling(1) on this thread, the device time in ms of k_iforest_build and k_iforest_score of
 * this thread's last forest call, from HIP events on its stream.  An event call that fails costs that measurement
 * (-1 in its slot) and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_iforest_set_profiling(int32_t on);
eao_status eao_iforest_last_kernel_ms(float* kernel_ms /* 2 */);
/* The same measurement inside k_iforest_build: the mean over the trees of the last call, in microseconds of the device's constant clock, of seeding the
 * generator, of the shuffle with the copy of the sample, and of the depth-first walk. */
eao_status eao_iforest_last_stage_us(double* stage_us /* 3 */);

/* ---- Object layer: the per-frame data association of Tracking step 10 (src/Tracking.cc:2036-2069) -----------------------------------------------------------
 * Object_2D::NoParaDataAssociation (src/Object.cc:728-962; called for one detection against every map object of its class, :260-277): the Wilcoxon rank-sum
 * test of a detection's map points against a map object's, and Object_Map::ComputeProjectRectFrame (:1606-1651; called per object at src/Tracking.cc:2049): the
 * bounding box of an object's projected points.  Both are pure functions of point lists and both are exact: integer counts, and the cv::Mat arithmetic
 * convention of DESIGN.md section 2 (csrc/object_assoc_internal.h).  The entries are stateless; each host thread has its own stream and
 * staging.  EAO_ERR_INVALID leaves every output untouched.  Two calls on the same arguments return the same bytes, on one thread or on several.
 *
 * The lists: detection d owns points det_start[d] .. det_start[d+1] - 1 of det_xyz, map object j points map_start[j] .. map_start[j+1] - 1 of map_xyz (3 floats
 * each; starts >= 0 and ascending).  They hold the GOOD points only -- not isBad() and not out_point (:737, :751) -- gathered in vector order; map_total[j] is
 * mvpMapObjectMappoints.size() with the bad ones, which upstream's sampling step is computed from (:779), so map_total[j] >= the list's length.  Pair p tests
 * detection pair_det[p] against map object pair_map[p]; pairs may repeat.
 *
 * eao_object_np_counts_batch: per pair mns = {m, n, step} and counts = {w_x_12, w_x_21, w_x_00, w_y_.., w_z_..} of :830-923 as integers (upstream's float counters
 * hold the same values: m * n < 2^24 under the bound below).  m = the detection's points, nGood = the map object's.
 *   m < 20 (:760) or otherwise nGood < 20 (:764)   n = nGood, step = 0 (upstream has not declared step), counts = 0
 *   nGood <= 3 m                                   n = nGood, step = 1 (:775, :826)
 *   nGood > 3 m                                    step = map_total / (3 m) (:779), n = ceil(nGood / step) (:802-808)
 *   m n (m + n + 1) > INT32_MAX                    n and step as in the two rows above, counts = 0: upstream's int product at :942 overflows (undefined)
 * eao_object_np_association_batch: per pair upstream's return value -- 0 (m < 20: go on with the t-tests), 1 (associated), 2 (failed, nGood < 20 included) -- or
 * EAO_OBJECT_NP_UNDEFINED where the int product overflows; the other pairs of the call are unaffected.  w (optional, 3 per pair) = w_x, w_y, w_z of :930-932 and
 * r (optional, 2 per pair) = r1, r2 of :942-943; zero for the pairs the counts do not decide.  Those pairs cost no device work and their points are not read.
 * Refused with EAO_ERR_INVALID: a negative count, starts that do not ascend, map_total below the list's length, a pair index out of range, and a NaN
 * coordinate in a list that a pair whose counts decide reads (upstream would count such a value in none of its three counters; infinities compare normally). */
#define EAO_OBJECT_NP_MIN_DET_POINTS 20         /* src/Object.cc:760 */
#define EAO_OBJECT_NP_MIN_MAP_POINTS 20         /* :764 */
#define EAO_OBJECT_NP_SAMPLE_RATIO 3            /* :776 */
#define EAO_OBJECT_NP_CRITICAL 1.282            /* :942 */
#define EAO_OBJECT_NP_VARIANCE_DIVISOR 12       /* :942 */
#define EAO_OBJECT_NP_HALF 0.5                  /* :942 */
#define EAO_OBJECT_NP_UNDEFINED 3
eao_status eao_object_np_counts_batch(int32_t n_det, const int32_t* det_start /* n_det+1 */, const float* det_xyz, int32_t n_map,
                                      const int32_t* map_start /* n_map+1 */, const float* map_xyz, const int32_t* map_total /* n_map */, int32_t n_pair,
                                      const int32_t* pair_det, const int32_t* pair_map, int32_t* mns /* n_pair x 3 */, uint32_t* counts /* n_pair x 9 */);
eao_status eao_object_np_association_batch(int32_t n_det, const int32_t* det_start /* n_det+1 */, const float* det_xyz, int32_t n_map,
                                           const int32_t* map_start /* n_map+1 */, const float* map_xyz, const int32_t* map_total /* n_map */, int32_t n_pair,
                                           const int32_t* pair_det, const int32_t* pair_map, int32_t* verdict /* n_pair */, float* w /* n_pair x 3 */,
                                           float* r /* n_pair x 2 */);
/* Object_Map::ComputeProjectRectFrame for a batch of map objects under one pose: map_xyz = GetWorldPos() of ALL of mvpMapObjectMappoints in vector order (the
 * function does not filter), Tcw = mCurrentFrame.mTcw (4x4 row-major), fx .. cy = the frame's intrinsics, cols and rows = the image's.  Per object rect = {x, y,
 * width, height} of mRectProject (:1650) and status:
 *   0  no points: upstream returns at :1631 and rect is untouched
 *   1  rect is written
 *   2  upstream is undefined and rect is untouched: a projection is a NaN (std::sort's ordering contract at :1634), or a clamped value (:1641-1648) or a
 *      difference of two lies outside int, where cv::Rect's float -> int conversion is undefined.  An infinite projection (z = 0 with x != 0) is defined.
 * uv (optional, 2 floats per point, indexed like the points): u and v of :1623-1624.  Refused with EAO_ERR_INVALID: a negative count, starts that do not
 * ascend. */
eao_status eao_object_project_rects_batch(int32_t n_map, const int32_t* map_start /* n_map+1 */, const float* map_xyz, const float* Tcw /* 16 */, float fx, float fy,
                                          float cx, float cy, int32_t cols, int32_t rows, int32_t* rect /* n_map x 4 */, uint8_t* status /* n_map */, float* uv);
/* Diagnostic (tools/bench_object_association.py): after eao_object_assoc_set_profiling(1) on this thread, the device time in ms of k_np_counts in this thread's
 * last rank-sum call that reached the device and of k_project_rects in its last rect call (-1 for a kernel that has not run since), from HIP events on its stream.  An event call that fails costs that measurement
 * (-1 in its slot) and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_object_assoc_set_profiling(int32_t on);
eao_status eao_object_assoc_last_kernel_ms(float* kernel_ms /* 2 */);

/* ---- Object layer: a frame's 2D objects, steps 2, 4, 5 and 6 of the object layer (src/Tracking.cc:1768-1973) -------------------------------------------------
 * What Tracking::TrackWithMotionModel makes of the detector's boxes before the data association: Tracking::AssociateObjAndPoints (:3031-3065), per box
 * Object_2D::ComputeMeanAndStandardFrame and RemoveOutliersByBoxPlot (src/Object.cc:61-157), the projection of the centre and the box of the feature points
 * (:1801-1854), and the removal of bad boxes (:1868-1973).  A pure function of the frame, bit for bit (csrc/frame_objects_internal.h):
 * one workgroup per (frame, box) compacts the box's keypoints in keypoint order, three lanes add the positions and the squares in that order, Q1 and Q3 come
 * from counting ranks, and the sequential second loop of step 6 runs on the host behind the download.  The entries are stateless; each host thread has its own
 * stream and staging.  EAO_ERR_INVALID leaves every output untouched.  Two calls on the same arguments return the same bytes, on one thread or on several.
 *
 * A frame: keypoint i has the undistorted coordinates kp_x[i], kp_y[i] (mvKeysUn[i].pt), mp_id[i] = -1 where mvpMapPoints[i] is NULL or isBad() (:3038, :3042)
 * and otherwise an id >= 0 that is equal for two keypoints exactly when they hold the same MapPoint, and mp_xyz[3 i ..] = GetWorldPos() (read only where
 * mp_id[i] >= 0).  Box k = {x, y, width, height} of mBoxRect (= mBox, src/Object.cc:53-56) with score[k] = mScore (may be a NaN).  Tcw: mCurrentFrame.mTcw, 4x4
 * row-major; cols, rows: the image's.
 *
 * A record per box, the frames' boxes back to back:
 *   n_assigned, sum_pos         Obj_c_MapPonits.size() and sum_pos_3d after step 2: the keypoints with a map point whose cvRound'ed position (nearest, ties to
 *                               even) has x <= px < x + width and y <= py < y + height (:3046), added in keypoint order, one float add per coordinate (:3059)
 *   boxplot_ran, q1, q3, max_th n_assigned >= 8 (:1782): Q1 = sorted z[n / 4], Q3 = sorted z[n * 3 / 4] over the camera-frame depths, max_th = (float)(Q3 + 1.5 IQR)
 *                               (src/Object.cc:134-139); zero where the boxplot did not run
 *   n                           the list's length after the points with z > max_th left it (:150), = mCountMappoint (:1807)
 *   pos, std                    _Pos = sum_pos / n -- the sum of step 2 over the count after the boxplot: the erase does not touch sum_pos_3d -- as
 *                               sum * (float)(1.0 / n) + 0.0f, and mStandar_x / y / z about it (:80-99).  n == 0: NaN, as upstream.
 *   center_2d                   point_center_2d (:1809-1816)
 *   has_feature_rect, feature_rect   n >= 4 (:1830) and mRectFeaturePoints = {x, y, width, height} (:1836-1853) over pMP->feature of the list: a map point that
 *                               several keypoints hold carries the coordinates of the LAST of them that lies in any box (:3053); zero otherwise
 *   num_overlaps                the other boxes l with bboxOverlapratioLatter(this, l) > 0.05 (:1870-1878)
 *   bad, on_edge                after both loops of :1868-1945; the caller erases the bad objects (:1949-1973).  on_edge is 0 where upstream leaves bOnEdge alone.
 * assigned / kept: the keypoint indices (within the frame) of Obj_c_MapPonits after step 2 / after the boxplot, in upstream's order; box b of the call owns
 * entries assigned_start[b] .. assigned_start[b + 1] - 1 (kept_start likewise; total boxes + 1 entries each).  A list buffer that is too short is
 * EAO_ERR_CAPACITY: assigned_start and kept_start are filled, nothing else is written.
 * Refused with EAO_ERR_INVALID: a non-finite keypoint, position (where mp_id >= 0), pose or intrinsic; |kp| >= 2^30 (upstream's float -> int conversions are
 * undefined there); a negative box width or height, a box field or an image size beyond 2^15 (the int areas stay in range); n_kp above
 * EAO_FRAME_OBJECTS_MAX_KEYPOINTS (the tracker's limit); n_box above EAO_FRAME_OBJECTS_MAX_BOXES; mp_id < -1; more than EAO_FRAME_OBJECTS_MAX_FRAMES frames, or a
 * batch whose lists could hold more than 2^30 entries (boxes times keypoints with a map point, summed over the frames): split such a call.  Zero-area boxes,
 * frames without keypoints and n_box == 0 are valid. */
#define EAO_FRAME_OBJECTS_MAX_KEYPOINTS 4096
#define EAO_FRAME_OBJECTS_MAX_BOXES 256
#define EAO_FRAME_OBJECTS_MAX_FRAMES 65535
typedef struct {
    int32_t n_kp;
    const float* kp_x;        /* n_kp */
    const float* kp_y;        /* n_kp */
    const int32_t* mp_id;     /* n_kp */
    const float* mp_xyz;      /* n_kp x 3 */
    int32_t n_box;
    const int32_t* boxes;     /* n_box x 4 */
    const float* score;       /* n_box */
    float Tcw[16];
    float fx, fy, cx, cy;
    int32_t cols, rows;
} eao_frame_objects_desc;
typedef struct {
    int32_t n_assigned, n;
    float sum_pos[3], pos[3], std[3];
    float q1, q3, max_th;
    int32_t boxplot_ran;
    float center_2d[2];
    int32_t has_feature_rect;
    int32_t feature_rect[4];
    int32_t num_overlaps, bad, on_edge;
} eao_frame_object_record; /* 100 bytes */
typedef struct {
    eao_frame_object_record* records; /* total boxes */
    int32_t* assigned_start;          /* total boxes + 1 */
    int32_t* assigned;
    int64_t assigned_cap;             /* in entries */
    int32_t* kept_start;              /* total boxes + 1 */
    int32_t* kept;
    int64_t kept_cap;
} eao_frame_objects_out;
eao_status eao_frame_objects_batch(int32_t n_frames, const eao_frame_objects_desc* frames, const eao_frame_objects_out* out);
/* a batch of one */
eao_status eao_frame_objects(const eao_frame_objects_desc* frame, const eao_frame_objects_out* out);
/* Diagnostic (tools/bench_frame_objects.py): after eao_frame_objects_set_profiling(1) on this thread, the device time in ms of k_frame_features, k_frame_objects
 * and k_frame_pack of this thread's last call that reached the device, from HIP events on its stream.  An event call that fails costs that measurement
 * (-1 in its slot) and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_frame_objects_set_profiling(int32_t on);
eao_status eao_frame_objects_last_kernel_ms(float* kernel_ms /* 3 */);

/* ---------------------------------------------------------------------------------------------------
 * object_cuboid: a map object's centre, deviations, bounds, poses, corners and scale -- Object_Map::ComputeMeanAndStandard (reference src/Object.cc:999-1235)
 * with both of its calls of Object_Map::UpdateObjPose (:2243-2303) -- on the device, one launch for a batch of objects, bit for bit what upstream's loops compute
 * (csrc/object_cuboid_internal.h holds the literal form; DESIGN.md section 4q states the order of every sum and every reading that OpenCV, Eigen and g2o leave
 * open).  Upstream calls it once per associated object per frame (src/Object.cc:718-719, :1593-1596, src/Tracking.cc:3136), after merges and splits (:1691-1699,
 * :2089, :2200-2201) and for every object of the map on every keyframe (LocalMapping::UpdateObject, src/LocalMapping.cc:771-794).  The entries are stateless;
 * each host thread has its own stream and staging.  EAO_ERR_INVALID leaves every output untouched.  Two calls on the same arguments return the same bytes, on
 * one thread or on several.
 *
 * An object: points = GetWorldPos() of mvpMapObjectMappoints in list order AFTER the erase of the bad ones (:1003-1024; include/eaofusion/ObjectMap.h erases),
 * centroids = mObjectFrame[i]->_Pos in list order, Ryaw = the nine floats of upstream's own expression over rotP / rotR / rotY (:2250-2260, row-major; no sin or
 * cos runs in the library), prev_cuboid_center = mCuboid3D.cuboidCenter before the call (read only when n_centroids >= 5).
 *
 * A record per object, stored whole:
 *   status                      EAO_OBJECT_CUBOID_EMPTY: n_points == 0, the return of :1050; sum_pos, center and standar hold what upstream holds there (0 and
 *                               NaNs) and every other field is zero: upstream leaves those members untouched.  Otherwise EAO_OBJECT_CUBOID_DONE.
 *   sum_pos, center, standar    mSumPointsPos (float adds in list order, :1020), mCenter3D = sum * (float)(1.0 / n) + 0.0f (:1027), mStandar_x / y / z (:1030-1048)
 *   center_standar[3]           mCenterStandar_x / y / z over the centroids (:1054-1068); n_centroids == 0 divides by zero as upstream does (NaN)
 *   center_standar_dis          mCenterStandar (:1220-1234)
 *   bounds_written, bounds      n_centroids < 5 (:1071): x_min, x_max, y_min, y_max, z_min, z_max of the world-frame points (:1095-1100).  Otherwise upstream leaves
 *                               them untouched: zero.  Among equal extrema (a -0.0f beside a +0.0f) the one with the smallest list position is taken.
 *   lenth, width, height        the object-frame scale (:1182-1184)
 *   rmax                        mCuboid3D.mfRMax (:1189-1217)
 *   Twobj, Twobj_without_yaw    the two float matrices of the SECOND UpdateObjPose (:1186), row-major; Converter::toSE3Quat of them is mCuboid3D.pose and
 *                               pose_without_yaw
 *   cuboid_center               (corner_2 + corner_8) / 2 (:1185)
 *   corners, corners_w          corner_1 .. corner_8 through pose (:1160-1167) and corner_1_w .. corner_8_w through pose_without_yaw (:1170-1177), both poses those
 *                               of the FIRST UpdateObjPose (:1128)
 *   pose_q, pose_t, pose_without_yaw_q, pose_without_yaw_t      the library's own Quaterniond(R) + normalizeRotation (x, y, z, w) and translation of the final poses
 * A NaN's sign and payload are nobody's contract.
 * Refused with EAO_ERR_INVALID before anything is written: a negative count; a null pointer where a count is positive; a non-finite point, centroid, Ryaw entry
 * or prev_cuboid_center; more than EAO_OBJECT_CUBOID_MAX_OBJECTS objects or more than 2^27 points and centroids in one call (split it).  n_points == 0 and
 * n_centroids == 0 are valid.  Finite inputs whose squares overflow float are computed, not refused. */
#define EAO_OBJECT_CUBOID_MAX_OBJECTS 65535
#define EAO_OBJECT_CUBOID_EMPTY 0
#define EAO_OBJECT_CUBOID_DONE 1
typedef struct {
    int32_t n_points;
    const float* points;          /* n_points x 3 */
    int32_t n_centroids;
    const float* centroids;       /* n_centroids x 3 */
    float Ryaw[9];
    double prev_cuboid_center[3];
} eao_object_cuboid_desc;
typedef struct {
    int32_t status, bounds_written;
    float sum_pos[3], center[3], standar[3];
    float center_standar[3], center_standar_dis;
    float bounds[6];
    float lenth, width, height;
    float rmax;
    int32_t reserved;             /* zero */
    float Twobj[16], Twobj_without_yaw[16];
    double cuboid_center[3];
    double corners[8][3], corners_w[8][3];
    double pose_q[4], pose_t[3];
    double pose_without_yaw_q[4], pose_without_yaw_t[3];
} eao_object_cuboid_rec; /* 752 bytes */
eao_status eao_object_cuboids_batch(int32_t n_obj, const eao_object_cuboid_desc* objs, eao_object_cuboid_rec* recs);
/* a batch of one */
eao_status eao_object_cuboids(const eao_object_cuboid_desc* obj, eao_object_cuboid_rec* rec);
/* Object_Map::WhetherOverlap (src/Object.cc:1954-1970) over every ordered pair of m objects, with the three overlap extents of
 * LocalMapping::WhetherOverlapObject (src/LocalMapping.cc:858-877): the matrix Tracking's step 10.3 (src/Tracking.cc:2093-2103) and the mapping thread walk with
 * m^2 scalar calls.  verdict[i * m + j] = 1 when i != j, eligible[i] and eligible[j] are non-zero and |dc| < l / 2 + l' / 2 holds on all three axes (`<` is
 * strict: touching boxes do not overlap); extents (optional) receives sum_half - dis per axis at 3 * (i * m + j), written only where the verdict is 1.
 * DealTwoOverlapObjs' decisions and the loops' early `break` stay with the caller; its erases (BigToSmall, DivideEquallyTwoObjs) are the BOX and SHRUNK rules
 * of eao_object_points_update_batch below.  Refused: a negative m or one above EAO_OBJECT_OVERLAP_MAX_ROWS, a null pointer where
 * m > 0, a non-finite field of a row. */
#define EAO_OBJECT_OVERLAP_MAX_ROWS 2048
typedef struct {
    double cuboid_center[3];      /* mCuboid3D.cuboidCenter */
    float lenth, width, height;   /* mCuboid3D.lenth / width / height */
    int32_t reserved;
} eao_object_overlap_row; /* 40 bytes */
eao_status eao_object_overlaps(int32_t m, const eao_object_overlap_row* rows, const uint8_t* eligible, uint8_t* verdict /* m * m */, float* extents /* optional, m * m * 3 */);
/* Diagnostic (tools/bench_object_cuboid.py): after eao_object_cuboid_set_profiling(1) on this thread, the device time in ms of k_object_cuboids and
 * k_object_overlaps of this thread's last calls that reached the device (-1 for a kernel that has not run since), from HIP events on its stream.  An event call
 * that fails costs that measurement and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_object_cuboid_set_profiling(int32_t on);
eao_status eao_object_cuboid_last_kernel_ms(float* kernel_ms /* 2 */);

/* ---------------------------------------------------------------------------------------------------
 * object_points: the update of a map object's point list (mvpMapObjectMappoints) on the device -- step 1, 3 and 4 of Object_Map::DataAssociateUpdate (reference
 * src/Object.cc:1364-1436, :1460-1535, :1538-1589), step 1 of Object_Map::MergeTwoMapObjs (:1766-1821) and the erase loops of BigToSmall (:2070-2087) and
 * DivideEquallyTwoObjs (:2096-2120) -- bit for bit what upstream's loops compute (csrc/object_points_internal.h holds the literal form; DESIGN.md section 4r
 * states why the growing list can be compared all pairs at once).  A desc is one (map object, source) pair; its stages run in upstream's order and each is
 * optional.  The entries are stateless; each host thread has its own stream and staging.  EAO_ERR_INVALID leaves every output untouched.  Two calls on the same
 * arguments return the same bytes, on one thread or on several.
 *
 *   1. change_gate != 0 (:1364-1436, upstream's Flags 2 and 3): the candidates and then the list are projected under Tcw and the intrinsics, the extrema of u and
 *      v are clamped (:1419-1426) and truncated as cv::Rect(float ...) does: rect2.  iou = bboxOverlapratio(project_rect1, rect2), iou2 =
 *      bboxOverlapratioFormer(rect2, box_rect).  (iou < 0.5) && (iou2 < 0.8), compared in double, a NaN ratio comparing false, is status REJECTED: upstream's
 *      `return false`, nothing else is computed.  A NaN projection, a conversion to int that is undefined, or no point at all (x_pt[0] of an empty vector) is
 *      status UNDEFINED: only the status is set.
 *   2. gate != NONE, per candidate j in order (:1460-1535, :1766-1821):
 *        RADIUS   fDis > th * rmax skips it (gate[j] = 0); fDis = sqrt of the float squares of center - p (:1465-1466), th = 0.9f when n_frames_after_push > 5 and
 *                 1.0f otherwise (:1468-1472)
 *        CUBOID   |pose.inverse() * p| in double against 1.1 * lenth / 2, 1.1 * width / 2, 1.1 * height / 2 (:1771-1774)
 *      count[j] = cand_count[j] + 1 where gate[j], cand_count[j] otherwise (what object_id_vector holds afterwards, :1492-1502).  A gated-in candidate is
 *      compared in list order with the list as it stands: the n_map entries, then those appended before it.  Equality is countNonZero(a - b) == 0: componentwise
 *      ==, so -0.0f equals +0.0f.  target[j] = the position in the final list of the first equal entry, or -1 for a candidate that is appended (and for one that
 *      is gated out).  list = the final list as (source, index) pairs, source 0 = the map list, 1 = the candidates.  sum_pos_appended = sum_pos plus the appended
 *      positions, float adds in append order (:1532).
 *   3. erase != NONE, over the list after stage 2 in list order:
 *        PROJECTION  (:1543-1588) only when box_off_edge != 0 (the caller's :1538-1541).  An entry whose count (map_count, or count[j] of an appended candidate)
 *                    exceeds 8 stays.  Otherwise it is erased when 0 < u < cols, 0 < v < rows and !box_rect.contains(Point2f(u, v)) (cvRound, half-open).
 *        BOX         (:2078-2081) erased when strictly inside bounds = x_min x_max y_min y_max z_min z_max
 *        SHRUNK      (:2105-2110) erased when strictly inside cuboid_center -+ (lenth / 2 - overlap / 2) on all three axes (the half-extents in float, the
 *                    bounds in double)
 *      erased[k] per list position, survivors = the (source, index) pairs that stay, in order; sum_pos = sum_pos_appended minus the erased positions, float
 *      subtractions in list order (:1577, PROJECTION only).  desc.survivors, where not NULL, receives the surviving positions, n_survivors x 3 floats: the
 *      `points` of an eao_object_cuboid_desc.
 * With a status other than DONE only the record is written.  A list entry that is the very MapPoint of a gated-in candidate shares its object_id_vector with it:
 * the caller that needs the incremented count in stage 3 passes it in map_count.
 * Refused with EAO_ERR_INVALID before anything is written: a negative count; a null pointer where a count is positive (map_count only with PROJECTION); a
 * non-finite coordinate, pose, intrinsic, bound, extent, centre, sum or rmax; an unknown gate or erase; cols, rows or a rect field outside -2^15 .. 2^15 (a
 * negative size); more than EAO_OBJECT_POINTS_MAX_DESCS descs or more than 2^27 points in one call (split it).  n_map == 0 and n_cand == 0 are valid. */
#define EAO_OBJECT_POINTS_MAX_DESCS 65535
#define EAO_OBJECT_POINTS_DONE 1
#define EAO_OBJECT_POINTS_REJECTED 2
#define EAO_OBJECT_POINTS_UNDEFINED 3
#define EAO_OBJECT_POINTS_GATE_NONE 0
#define EAO_OBJECT_POINTS_GATE_RADIUS 1
#define EAO_OBJECT_POINTS_GATE_CUBOID 2
#define EAO_OBJECT_POINTS_ERASE_NONE 0
#define EAO_OBJECT_POINTS_ERASE_PROJECTION 1
#define EAO_OBJECT_POINTS_ERASE_BOX 2
#define EAO_OBJECT_POINTS_ERASE_SHRUNK 3
#define EAO_OBJECT_POINTS_KEEP_COUNT 8           /* src/Object.cc:1555: a count above it keeps the point */
#define EAO_OBJECT_POINTS_EDGE_PIXELS 25         /* :1538-1541: the caller's box_off_edge */
typedef struct {
    int32_t change_gate, gate, erase, box_off_edge;
    int32_t n_map, n_cand;
    const float* map_points;      /* n_map x 3: GetWorldPos() of mvpMapObjectMappoints in list order */
    const int32_t* map_count;     /* n_map: object_id_vector[mnId], 0 where absent (PROJECTION only) */
    const float* cand_points;     /* n_cand x 3 */
    const int32_t* cand_count;    /* n_cand: object_id_vector[mnId] before the call, 0 where absent */
    float Tcw[16];                /* row-major */
    float fx, fy, cx, cy;
    int32_t cols, rows;
    int32_t project_rect1[4], box_rect[4];      /* x y width height */
    float center[3], rmax;        /* mCenter3D, mCuboid3D.mfRMax (RADIUS) */
    int32_t n_frames_after_push;  /* mObjectFrame.size() after :1451 (RADIUS) */
    float lenth, width, height;   /* of the cuboid the stage reads: this object's (CUBOID), the other one's (SHRUNK) */
    double pose_q[4], pose_t[3];  /* mCuboid3D.pose, x y z w (CUBOID) */
    double cuboid_center[3];      /* the other object's (SHRUNK) */
    float bounds[6];              /* the other object's (BOX) */
    float overlap[3];             /* (SHRUNK) */
    float sum_pos[3];             /* mSumPointsPos before the call */
    int32_t reserved;             /* zero */
    float* survivors;             /* optional, (n_map + n_cand) x 3 */
} eao_object_points_desc;
typedef struct {
    int32_t status;
    int32_t n_gated, n_appended, n_list, n_erased, n_survivors;
    int32_t rect2[4];
    float iou, iou2;
    float sum_pos_appended[3], sum_pos[3];
    int32_t reserved[2];          /* zero */
} eao_object_points_rec; /* 80 bytes */
typedef struct {
    eao_object_points_rec* rec;
    uint8_t* gate;                /* n_cand */
    int32_t* target;              /* n_cand */
    int32_t* count;               /* n_cand */
    int32_t* list;                /* (n_map + n_cand) x 2, n_list pairs written */
    uint8_t* erased;              /* n_map + n_cand, n_list written */
    int32_t* survivors;           /* (n_map + n_cand) x 2, n_survivors pairs written */
} eao_object_points_out;
eao_status eao_object_points_update_batch(int32_t n, const eao_object_points_desc* descs, const eao_object_points_out* outs);
/* a batch of one */
eao_status eao_object_points_update(const eao_object_points_desc* desc, const eao_object_points_out* out);
/* Diagnostic (tools/bench_object_points.py): after eao_object_points_set_profiling(1) on this thread, the device time in ms of k_object_points_match (-1 where
 * the call ran fused) and k_object_points (or k_object_points_finish) of this thread's last call that reached the device, from HIP events on its stream.  An
 * event call that fails costs that measurement and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_object_points_set_profiling(int32_t on);
eao_status eao_object_points_last_kernel_ms(float* kernel_ms /* 2 */);

/* ---------------------------------------------------------------------------------------------------
 * object_chain: the three numeric steps of Object_Map::DataAssociateUpdate (reference src/Object.cc:1352-1601) in ONE device call -- the point update above
 * (stages 1-3 of eao_object_points_update_batch), the erase of the bad points (:1003-1024), ComputeMeanAndStandard with both UpdateObjPose calls
 * (eao_object_cuboids_batch) and the isolation forest (:1239-1348, eao_object_iforest_outliers_batch) over the list the cuboid saw.  One upload, one download and
 * one wait on the stream per call; the list a stage leaves is read by the next one from device memory, and no count travels to the host in between.  Every
 * output is, bit for bit, what the three entries return when the caller chains them by hand (csrc/object_chain_internal.h).  The entries
 * are stateless; each host thread has its own stream and staging.  EAO_ERR_INVALID leaves every output untouched.  Two calls on the same arguments return the
 * same bytes, on one thread or on several.
 *
 * A desc:
 *   points                an eao_object_points_desc; its `survivors` is ignored here
 *   map_bad, cand_bad     n_map and n_cand bytes: isBad() of every point (a non-zero byte is a bad point)
 *   cand_alias            optional, n_cand entries: the list position < n_map of the entry that is the very MapPoint of candidate j, or -1.  Upstream's step 3
 *                         raises object_id_vector of a gated-in candidate before step 4 reads it (:1550-1559): with cand_alias the PROJECTION erase reads, for list
 *                         entry k, map_count[k] plus the number of gated-in candidates whose alias is k (the entry's host half forms the sum from the same gate
 *                         rule the device runs; integers only).  NULL gives exactly stage 3 of eao_object_points_update_batch.
 *   n_centroids, centroids, Ryaw, prev_cuboid_center        the cuboid's inputs as in eao_object_cuboid_desc (centroids = mObjectFrame[i]->_Pos AFTER step 2's push)
 *   class_id, bi_forest   mnClass and the file-level flag biForest (:1241)
 * Per desc, in upstream's order:
 *   1-3.  the point update: out.points receives what eao_object_points_update_batch writes (rec.sum_pos stays what stage 3 computed; upstream sums anew at :1001
 *         and so does the cuboid record).  A status other than DONE writes the points record and nothing else, and the stages behind cost no device work worth
 *         naming: their workgroups leave at once.
 *   4.    the survivors whose bad flag is set leave, in order: `final` receives the list of the cuboid and of the forest as (source, index) pairs, rec.n_final
 *         their number.
 *   5.    cuboid: the eao_object_cuboid_rec of that list (EMPTY when n_final == 0).
 *   6.    forest: the object runs when bi_forest is set, its class is none of 75 / 64 / 65 and n_final >= 30; the device decides this from n_final.  Then
 *         Build(50, 12345, data, n_final / 2); the device returns the total path length per final position and the entry's host half finishes as
 *         eao_object_iforest_outliers_batch does (libm's pow, then the threshold).  forest_flags per final position (1 = erase), rec.removed their number, scores
 *         (optional) the anomaly scores, -1.0 where the forest was skipped.  rec.forest_status: SKIPPED, DONE, or FAILED where upstream's Build returns false
 *         (flags all zero, scores -1.0).
 * Refused with EAO_ERR_INVALID before anything is written: everything the three entries refuse; map_bad or cand_bad NULL where its count is positive; an alias
 * outside -1 .. n_map - 1; an output pointer that is NULL where its list can be non-empty; and a desc whose forest may run (bi_forest set, class not exempt) with
 * n_map + n_cand > EAO_IFOREST_MAX_POINTS: the true count is only known on the device, and the bound is the honest check.
 * Out of scope: the order of :718-719 (forest, erase, then cuboid; RefineObjects of include/eaofusion/ObjectMap.h stays as it is): its erase needs the flag on
 * the device, and the flag is pow(2, x) > th with libm's pow, which the device does not have bit for bit.  A handle that keeps lists resident across frames:
 * local bundle adjustment moves the points between frames.  MergeTwoMapObjsPoints, BigToSmall and DivideEquallyTwoObjs: no chain follows them upstream. */
#define EAO_OBJECT_CHAIN_FOREST_SKIPPED 0
#define EAO_OBJECT_CHAIN_FOREST_DONE 1
#define EAO_OBJECT_CHAIN_FOREST_FAILED 2
typedef struct {
    eao_object_points_desc points;
    const uint8_t* map_bad;       /* n_map */
    const uint8_t* cand_bad;      /* n_cand */
    const int32_t* cand_alias;    /* optional, n_cand */
    int32_t n_centroids;
    int32_t class_id;
    const float* centroids;       /* n_centroids x 3 */
    float Ryaw[9];
    int32_t bi_forest;
    double prev_cuboid_center[3];
} eao_object_chain_desc;
typedef struct {
    int32_t n_final;
    int32_t forest_status;
    int32_t removed;
    int32_t reserved;             /* zero */
} eao_object_chain_rec; /* 16 bytes */
typedef struct {
    eao_object_points_out points;
    eao_object_chain_rec* rec;
    int32_t* final;               /* (n_map + n_cand) x 2, n_final pairs written */
    eao_object_cuboid_rec* cuboid;
    uint8_t* forest_flags;        /* n_map + n_cand, n_final written */
    double* scores;               /* optional, n_map + n_cand, n_final written */
} eao_object_chain_out;
eao_status eao_object_update_chain_batch(int32_t n, const eao_object_chain_desc* descs, const eao_object_chain_out* outs);
/* a batch of one */
eao_status eao_object_update_chain(const eao_object_chain_desc* desc, const eao_object_chain_out* out);
/* Diagnostic (tools/bench_object_chain.py): after eao_object_chain_set_profiling(1) on this thread, the device time in ms of the chain's kernels in this thread's
 * last call that reached the device, from HIP events on its stream: k_object_points_match (-1 where the call ran fused), k_object_points (or
 * k_object_points_finish), k_object_chain_plan, k_object_cuboids, k_iforest_build and k_iforest_score (-1 where no desc's forest could run).  An event call that
 * fails costs that measurement and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_object_chain_set_profiling(int32_t on);
eao_status eao_object_chain_last_kernel_ms(float* kernel_ms /* 6 */);

/* ---------------------------------------------------------------------------------------------------
 * yolox: what YOLOX::Detect (reference src/YOLOX.cc:369-410) does AROUND the network, on the device.  The network itself is the integrator's engine; it reads
 * the blob and writes the head output in HBM, and nothing of either crosses to the host.
 *   in front   StaticResize (:51-62): r = min(S / (cols * 1.0), S / (rows * 1.0)) stored as float, unpad = (int)(r * cols) -- a float product truncated: a
 *              1064-wide frame gives 639 columns -- cv::resize's 8-bit bilinear form into the top-left corner of an S x S canvas of 114;
 *              BlobFromImage (:211-233): B and R swapped in place, (((float)v) / 255.0f - mean[c]) / std[c] with float mean / std, HWC -> CHW: 3 x S x S floats;
 *              and, where wanted, the grey image Tracking::GrabImageRGBD makes of the same frame (src/Tracking.cc:324-330; OpenCV 3.x:
 *              (R 4899 + G 9617 + B 1868 + 8192) >> 14) in a pitched buffer eao_orb_extract_batch_device reads directly.
 *   behind     DecodeOutputs (:235-274): GenerateGridsAndStride (:64-77, strides 8 / 16 / 32), GenerateYoloxProposals (:166-209, box_prob = objectness * cls
 *              kept when > conf), the descending sort (:85-130), NmsSortedBboxes (:132-164, class-agnostic, inter / union > nms), the division by `scale` (the
 *              float r above) and the clip to [0, img_w - 1] x [0, img_h - 1] (:258-272).
 * Two things are not the reference's own, and the library says when they matter:
 *   exp        w and h are exp(feat) * stride (:183-184).  That call is glibc's expf, which is not correctly rounded and is chosen by CPU at run time: the
 *              reference is not pinned there.  The library defines both through the double-precision exponential rounded once to float.
 *   ties       the reference's quicksort orders proposals of EQUAL prob by its own swaps; the library orders them by proposal index (anchor * classes + class)
 *              and reports n_tied, the number of proposals that share their prob with another one.  When n_tied > 0 the reference's order may differ;
 *              include/eaofusion/YOLOX.h then decodes on the host, as it does when a frame has more than max_proposals proposals.
 * Calls on one handle are serialised; handles are independent (one stream each). */
#define EAO_YOLOX_INPUT_SIZE 640              /* include/YOLOX.h:71-72 */
#define EAO_YOLOX_NUM_CLASSES 80              /* src/YOLOX.cc:168 */
#define EAO_YOLOX_PAD 114                     /* :59 */
#define EAO_YOLOX_DEFAULT_PROPOSALS 4096
#define EAO_YOLOX_MAX_PROPOSALS 16384
#define EAO_YOLOX_MAX_INPUT_SIZE 2048
#define EAO_YOLOX_MAX_CLASSES 1024
#define EAO_YOLOX_MAX_BATCH 256
#define EAO_YOLOX_MAX_IMAGE 16384
typedef struct eao_yolox eao_yolox;
typedef struct {
    int32_t input_size;       /* S: square, a multiple of 32 (the reference's 640) */
    int32_t num_classes;      /* 80: a head row is 5 + num_classes floats */
    float conf_thresh;        /* BBOX_CONF_THRESH 0.3 passed on as a float (include/YOLOX.h:34, src/YOLOX.cc:241); >= 0 */
    float nms_thresh;         /* NMS_THRESH 0.65 as a float (include/YOLOX.h:33, src/YOLOX.cc:247) */
    int32_t max_proposals;    /* per frame; the reference has no cap: more is EAO_ERR_CAPACITY */
    int32_t max_batch;        /* frames per call */
} eao_yolox_cfg;
typedef struct {
    float x, y, w, h, prob;   /* Object::rect and prob (include/YOLOX.h:36-46) */
    int32_t label;
} eao_yolox_object;
/* the reference's literals: 640, 80, 0.3f, 0.65f; max_proposals 4096, max_batch 1 */
void eao_yolox_cfg_default(eao_yolox_cfg* cfg);
eao_status eao_yolox_create(const eao_yolox_cfg* cfg, eao_yolox** out);
void eao_yolox_destroy(eao_yolox* h);
/* StaticResize + BlobFromImage (:51-62, :211-233) of `batch` host frames of interleaved 8-bit colour, rows `stride` bytes apart (>= 3 * width), frames
 * frame_stride bytes apart: one upload, one kernel.  The blob stays in the handle (eao_yolox_buffers names it, eao_yolox_blob copies it out).  The blob reads
 * byte 2 - c of a pixel for channel c whatever `rgb` says, as the reference does; rgb (Tracking::mbRGB) only selects RGB2GRAY or BGR2GRAY for the grey image
 * (:324-330), which is written to `gray` (optional host array, batch x height rows of gray_stride >= width bytes).  A frame without a letterbox (an unpadded
 * size of 0, where cv::resize asserts) is EAO_ERR_INVALID; every EAO_ERR_INVALID leaves the outputs untouched. */
eao_status eao_yolox_preprocess(eao_yolox* h, const uint8_t* frames, int32_t width, int32_t height, int32_t stride, int64_t frame_stride, int32_t batch, int32_t rgb,
                                uint8_t* gray, int32_t gray_stride);
/* The same over device pointers, asynchronous on `stream` (a hipStream_t; NULL = the null stream): d_blob receives batch x 3 x S x S floats (16-byte
 * aligned), d_gray (optional, 4-byte aligned) batch x height rows of gray_stride bytes, gray_stride a multiple of 64 -- the bytes of a row behind `width` are
 * written too (zeros).  One upload of the colour frame feeds the detector and, through d_gray, eao_orb_extract_batch_device on the same stream. */
eao_status eao_yolox_preprocess_device(eao_yolox* h, const uint8_t* d_frames, int32_t width, int32_t height, int32_t stride, int64_t frame_stride, int32_t batch,
                                       int32_t rgb, float* d_blob, uint8_t* d_gray, int32_t gray_stride, void* stream);
/* DecodeOutputs (:235-274) of `batch` head outputs (host array, batch x anchors x (5 + num_classes) floats; anchors = sum of (S / stride)^2) for images of
 * img_w[f] x img_h[f] pixels (`scale` is their r).  objects: batch x cap records, frame f's at objects + f * cap, in the order the reference leaves them
 * (descending prob); n[f] of them; n_proposals[f]: the proposals before suppression; n_tied[f]: see above.
 * EAO_ERR_CAPACITY: a frame has more than max_proposals proposals -- n_proposals holds the true counts of every frame and nothing else is written -- or more
 * than cap objects -- n and n_proposals hold the counts and no object is written. */
eao_status eao_yolox_decode(eao_yolox* h, const float* prob, int32_t batch, const int32_t* img_w, const int32_t* img_h, eao_yolox_object* objects, int32_t cap,
                            int32_t* n, int32_t* n_proposals, int32_t* n_tied);
/* The same over a head output in HBM, enqueued on `stream` behind whatever wrote it, and waited for: the result arrays are host arrays. */
eao_status eao_yolox_decode_device(eao_yolox* h, const float* d_prob, int32_t batch, const int32_t* img_w, const int32_t* img_h, eao_yolox_object* objects,
                                   int32_t cap, int32_t* n, int32_t* n_proposals, int32_t* n_tied, void* stream);
/* The handle's own device buffers and stream, for an engine that runs between eao_yolox_preprocess and eao_yolox_decode_device (DoInference, :350-366, without its
 * two copies): d_blob max_batch x 3 x S x S floats, d_prob max_batch x anchors x (5 + num_classes) floats.  Any of the three may be NULL. */
eao_status eao_yolox_buffers(eao_yolox* h, float** d_blob, float** d_prob, void** stream);
/* `batch` head outputs at d_prob copied to the host array prob, behind whatever `stream` holds: what the host decode of include/eaofusion/YOLOX.h reads when the
 * library reports a tie or an overflow. */
eao_status eao_yolox_head(eao_yolox* h, const float* d_prob, int32_t batch, float* prob, void* stream);
/* Inspection: the blob of frame `frame` of the last eao_yolox_preprocess (3 x S x S floats), and the sorted proposals of frame `frame` of the last decode that
 * did not overflow (unscaled boxes x0, y0, w, h of :185-199; proposals may be NULL to ask for the count). */
eao_status eao_yolox_blob(eao_yolox* h, int32_t frame, float* blob);
eao_status eao_yolox_proposals(eao_yolox* h, int32_t frame, eao_yolox_object* proposals, int32_t cap, int32_t* n);
/* Diagnostic (tools/bench_yolox.py): after eao_yolox_set_profiling(h, 1), the device time in ms of k_yolox_pre, k_yolox_proposals, k_yolox_rank, k_yolox_mask and
 * k_yolox_scan of the handle's last calls (-1 for a kernel that has not run since), from HIP events on the call's stream; eao_yolox_preprocess_device then waits
 * for its kernel.  An event call that fails costs that measurement and never fails the product call.  EAO_ERR_INVALID when no slot is measured. */
eao_status eao_yolox_set_profiling(eao_yolox* h, int32_t on);
eao_status eao_yolox_last_kernel_ms(eao_yolox* h, float* kernel_ms /* 5 */);

/* ---- The detector network: the engine YOLOX::YOLOX deserialises (src/System.cc:112, src/YOLOX.cc:7-48) and DoInference runs (:331-367) ---------------------------
 * The reference's engine is a TensorRT blob.  Here the network is a graph of convolutions read from a model file (csrc/detnet_internal.h states the format, the
 * checks and the arithmetic; eao_fusion_amd/detnet.py writes it, tools/export_detnet.py makes it from a torch module): FOCUS, CONV (k 1 or 3, stride 1 or 2, bias,
 * none / SiLU / sigmoid, optional residual), MAXPOOL and UPSAMPLE2 over channel ranges of NHWC tensors.  The prediction convolutions write straight into the head
 * output eao_yolox_decode_device reads: anchors x (5 + classes) floats, strides 8, 16, 32 in that order (:64-77, :166-209).
 * A convolution is DEFINED as acc = bias, then acc = fmaf(x, w, acc) over ky, kx, ci ascending with +0.0f outside the map; sigmoid as
 * 1.0f / (1.0f + exp(-x)) with the exponential of the eao_yolox_* section.  The f32-input MFMA of gfx950 computes exactly that chain, so the output is the
 * host walk's (tools/detnet_walk.cpp), bit for bit.  Grouped and depthwise convolutions (YOLOX-nano, YOLOX-tiny) are refused.
 * Arguments and the file are checked before the device is touched: a bad file is EAO_ERR_INVALID with a message and never an out-of-range read.
 * Calls on one handle are serialised; handles are independent. */
typedef struct eao_detnet eao_detnet;
typedef struct {
    int32_t classes, anchors;         /* a head row is 5 + classes floats; anchors = sum of (S / stride)^2, 0 for a model without a head */
    int32_t tensors, ops;
    int32_t input_size, max_batch;
    int64_t weight_bytes;             /* on the device */
    int64_t activation_bytes;         /* the one allocation all intermediate tensors of max_batch frames live in */
    double flops;                     /* of one frame: 2 per multiply-add of the convolutions */
} eao_detnet_desc;
/* YOLOX::YOLOX (src/YOLOX.cc:7-48) over a model in memory (`bytes` bytes; it is not referenced after the call) for an input of input_size x input_size (a
 * multiple of 32: tensors are sized by their downscale, one file serves every size) and up to max_batch frames per call. */
eao_status eao_detnet_create(const void* model, int64_t bytes, int32_t input_size, int32_t max_batch, eao_detnet** out);
/* The same from a file, as the reference's constructor reads its engine file (:9-20). */
eao_status eao_detnet_create_from_file(const char* path, int32_t input_size, int32_t max_batch, eao_detnet** out);
/* YOLOX::~YOLOX (include/YOLOX.h:92, src/YOLOX.cc:43-49). */
void eao_detnet_destroy(eao_detnet* net);
/* What DoInference asks its engine (:333-347: the bindings, their types, getMaxBatchSize) and what the caller sizes d_prob by (output_size, src/YOLOX.cc:34-39). */
eao_status eao_detnet_info(const eao_detnet* net, eao_detnet_desc* info);
/* DoInference (:331-367) without its two copies: `batch` blobs of 3 x S x S floats at d_blob -> batch head outputs at d_prob, both in HBM; a sequence of
 * launches on `stream` (a hipStream_t; NULL = the null stream), asynchronous unless profiling is on.  d_prob may be NULL for a model without a head.
 * The handle's activations are written by the launches: a forward on another stream has to be ordered behind the previous one by the caller. */
eao_status eao_detnet_forward(eao_detnet* net, const float* d_blob, float* d_prob, int32_t batch, void* stream);
/* Inspection (the per-layer tests; the reference has no counterpart, its engine is opaque behind context->enqueue, :359): tensor `tensor` of frame `frame` of the
 * last forward, H x W x C floats (NHWC); waits for the device.  eao_detnet_set_tensor fills one: the
 * caller's input tensors of a single-op graph, or the channels of a tensor no op writes (they keep what they are given). */
eao_status eao_detnet_tensor(eao_detnet* net, int32_t tensor, int32_t frame, float* out);
eao_status eao_detnet_set_tensor(eao_detnet* net, int32_t tensor, int32_t frame, const float* in);
/* Diagnostic (tools/bench_detnet.py): after eao_detnet_set_profiling(net, 1) a forward records a HIP event around every op and waits; eao_detnet_last_op_ms
 * gives the device time in ms of each op of the last forward (cap >= ops; -1 where not measured).  An event call that fails costs that measurement and never
 * fails the product call (the reference runs context->enqueue, :359, untimed).  EAO_ERR_INVALID when nothing is measured. */
eao_status eao_detnet_set_profiling(eao_detnet* net, int32_t on);
eao_status eao_detnet_last_op_ms(eao_detnet* net, float* op_ms, int32_t cap);

/* The value of EAO_ABI_VERSION the library was built with. Bumped whenever an entry point's parameter list or a struct's layout changes (round 3
 * changed eao_tracker_track_local_map and eao_track_result in place); a caller compiled against another version must not call into the library.
 * Result structs are zero-initialised by the caller (`eao_track_result R = {0};`) before their array pointers are set: a pointer member the
 * caller's header does not know yet then reads as NULL = "not wanted". */
#define EAO_ABI_VERSION 6
int32_t eao_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* EAO_FUSION_H_ */
