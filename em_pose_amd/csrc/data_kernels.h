// Launch interfaces of the kernels around the model: synthetic sensors, root frame, resampling, sensor noise, offset
// statistics, placement search, metrics, temporal metrics, pose smoothing (sensor_sample.hip, root_frame.hip, resample.hip,
// sensor_noise.hip, offset_stats.hip, placement.hip, metrics.hip, temporal.hip, smooth.hip).
// Internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

// Synthetic sensor sampling (sensor_sample.hip): the frames of virtual_sensors_kernel plus the per-subject offsets,
// pos_synth = pos + ori . local, ori_synth = ori . r, in one launch; and the fold of the reverse, which turns the
// cotangents of the six outputs into those of (pos, ori) for launch_sensors_vjp.
constexpr int SAMPLE_LOCAL_NONE = 0;     // EMPOSE_SAMPLE_LOCAL_* (include/empose_hip.h)
constexpr int SAMPLE_LOCAL_WINDOW = 1;   // local [N][M][3]
constexpr int SAMPLE_LOCAL_FRAME = 2;    // local [N * F][M][3]
struct SampleSensorsArgs {
  const float* vertices;   // [T][V][3], T = N * F
  const int* center; const int* helper; const int* deg; const int* faces;   // as VirtualSensorArgs
  const float* local;      // by mode, or nullptr (SAMPLE_LOCAL_NONE)
  const float* r;          // [N][M][3][3] or nullptr (identity)
  float* pos; float* ori; float* normals;                   // [T][M][3], [T][M][9], [T][M][3], each or nullptr
  float* pos_synth; float* ori_synth; float* normal_synth;  // likewise
  int T, F, V, M, max_deg, mode;
};
hipError_t launch_sample_sensors(const SampleSensorsArgs& a, hipStream_t stream);
// One slab of T frames whose first frame is frame t0 of the batch (t0 selects the window of local and r); the pointers
// of the cotangents and of the outputs start at the slab.  d_pos_out is written when d_pos or d_pos_synth is given,
// d_ori_out when any of d_ori, d_ori_synth, d_normal_synth or (mode != NONE and d_pos_synth) is.
struct SampleFoldArgs {
  const float* d_pos; const float* d_ori;                                        // un-offset outputs, each or nullptr
  const float* d_pos_synth; const float* d_ori_synth; const float* d_normal_synth;   // each or nullptr
  const float* local; const float* r;   // whole batch, as SampleSensorsArgs
  float* d_pos_out; float* d_ori_out;   // [T][M][3], [T][M][9], each or nullptr
  int T, t0, F, M, mode;
};
hipError_t launch_sample_fold(const SampleFoldArgs& a, hipStream_t stream);

// Root normalisation and its vector-Jacobian product (root_frame.hip).  T frames in segments of seg_len rows; the root
// axis-angles are the first three columns of rows of ld_root floats.  `flags`: what happens to the translation.
constexpr int ROOT_FRAME_ROTATE = 1;     // trans_out = R_0^T trans
constexpr int ROOT_FRAME_SUBTRACT = 2;   // ... minus the first frame's (rotated) translation
constexpr int ROOT_FRAME_SUMS = 9;       // floats per wave of the reverse in `part`
struct RootFrameArgs {
  const float* root; int ld_root;
  const float* trans;                              // [T][3], read when flags != 0
  float* root_out; float* trans_out;               // forward: [T][3], [T][3] (flags != 0)
  const float* d_root_out; const float* d_trans_out;   // reverse: [T][3] each or nullptr
  float* g_root; float* g_trans;                   // reverse: [T][3]; g_trans is written when d_trans_out is given
  float* part;                                     // reverse: [root_frame_vjp_waves(T, seg_len)][ROOT_FRAME_SUMS]
  int T, seg_len, rod_conv, flags;
};
long root_frame_vjp_waves(int T, int seg_len);
hipError_t launch_root_frame_fwd(const RootFrameArgs& a, hipStream_t stream);
hipError_t launch_root_frame_vjp(const RootFrameArgs& a, hipStream_t stream);

// Resampling of a ragged batch of sequences to another frame rate (resample.hip).  One entry per sequence; the layout is
// that of empose_resample_seq (include/empose_hip.h).  Output rows are packed: out_row[s + 1] = out_row[s] + f_out[s].
struct ResampleSeq {
  int in_row, f_in, out_row, f_out;
  double fps_in, fps_out;
};
struct ResampleArgs {
  const ResampleSeq* seqs; int S;   // device table
  const float* in; int ld_in;       // rows of ld_in floats; the first 3 * n (rotations) or n (positions) columns are read
  float* out; int ld_out;
  int n;                            // joints per row (rotations) or channels (positions)
  long out_rows;                    // sum of f_out
  double* ws;                       // positions: [input rows][n] spline derivatives
};
hipError_t launch_resample_rotations(const ResampleArgs& a, hipStream_t stream);
hipError_t launch_resample_positions(const ResampleArgs& a, hipStream_t stream);

// Sensor-noise augmentation (sensor_noise.hip): one launch writes the noisy copies of [N][F][M * 3] positions and, when
// suppressing, [N][F][M * 9] orientations and [N][F][M * 3] normals, from a plan in device memory.
constexpr int SENSOR_NOISE_SPHERICAL = 0;   // EMPOSE_SENSOR_NOISE_* (include/empose_hip.h)
constexpr int SENSOR_NOISE_SUPPRESS = 1;
struct SensorNoiseArgs {
  const float* pos; const float* ori; const float* normal;   // ori, normal: suppression only
  float* pos_out; float* ori_out; float* normal_out;
  const int* start;                                // [N] first affected frame of a window
  const int* sensor;                               // suppression: [N][K], spherical: [K]
  const float* u_r; const float* theta; const float* phi;   // spherical: [N][window_len][K]
  int N, F, M, K, window_len, mode, thigh_a, thigh_b;
  float max_r, mask_value;
};
hipError_t launch_sensor_noise(const SensorNoiseArgs& a, hipStream_t stream);

// Per-subject sensor offsets from calibration recordings (offset_stats.hip): the inverse of launch_sample_sensors.  Per
// frame f and sensor m, with (pos, ori) the frame of sensor_frame.h on the ground-truth mesh and (p, R) the real reading,
//   o = ori^T (p - pos),   Q = ori^T R,
// and per (group, sensor) over the group's frames with mask == 1: the mean and the sample covariance of o, and the
// rotation closest to the mean of Q.  A group is a run of consecutive frames; the layout of a row is that of
// empose_offset_group (include/empose_hip.h).
constexpr int OFFSET_STATS_CHUNK = 256;   // frames per workgroup of the first pass, counted from the group's first frame
constexpr int OFFSET_STATS_SUMS = 19;     // count | sum o (3) | sum o o^T xx xy xz yy yz zz | sum Q (9)
struct OffsetGroup {
  int first_frame, n_frames;
};
struct OffsetStatsArgs {
  const float* vertices;   // [T][V][3]
  const int* center; const int* helper; const int* deg; const int* faces;   // as VirtualSensorArgs
  const float* p; const float* R;   // [T][M][3], [T][M][9]
  const float* masks;               // [T][M] or nullptr (every frame counts)
  const OffsetGroup* groups; int G; // device table
  double* sums;                     // [n_chunks][M][OFFSET_STATS_SUMS], a group's chunks after those of the groups before it
  float* local_f; float* q_f;       // [T][M][3], [T][M][9] or nullptr; written for the frames of the groups only
  float* means; float* covs; float* r; float* r_trace; int* counts;   // [G][M][3], [G][M][9], [G][M][9], [G][M], [G][M]
  int T, V, M, max_deg;
  int n_chunks;                     // sum over the groups of ceil(n_frames / OFFSET_STATS_CHUNK)
};
hipError_t launch_offset_stats(const OffsetStatsArgs& a, hipStream_t stream);

// Sensor placement search (placement.hip): which vertex does a sensor sit over?  Per sensor m and candidate vertex c, over
// the frames of a group with mask == 1,
//   score[m][c] = sum_f |p_f(m) - x_f(c)|^2 / n,   best[m] = the candidate with the lowest score (the lowest id on a tie).
// A call accumulates one slab of T frames into running sums; groups and slabs are the caller's loop.
constexpr int PLACEMENT_CHUNK = 64;     // frames per workgroup of the accumulation, counted from the slab's first frame
constexpr int PLACEMENT_SENSORS = 12;   // sensors a lane carries at a time; more take another grid row
struct PlacementArgs {
  const float* vertices;   // [T][V][3]
  const float* p;          // [T][M][3]
  const float* masks;      // [T][M] or nullptr (every frame counts)
  const int* cand;         // [C] ascending vertex ids, or nullptr (C == V, candidate c is vertex c)
  double* part;            // [ceil(T / PLACEMENT_CHUNK)][M][C] the chunks' sums (accumulate only)
  double* sums;            // [M][C] running sums of squared distances
  int* counts;             // [M] running numbers of counting frames
  float* score;            // finish: [M][C]
  int* best;               // finish: [M] vertex id, -1 when no frame counts
  float* best_score;       // finish: [M]
  int T, V, M, C;
};
hipError_t launch_placement_accumulate(const PlacementArgs& a, hipStream_t stream);
hipError_t launch_placement_finish(const PlacementArgs& a, hipStream_t stream);

struct MetricsArgs {
  const float* joints_gt; const float* joints_hat;   // [T][22][3]
  const float* pose_gt; const float* pose_hat;       // [T][63] body axis-angles (no root) or nullptr
  double* rows;                                      // [T][65] = 22 distances | 22 aligned distances | 21 angles (deg)
  int parents[22];
  int T;
};
hipError_t launch_metrics_rows(const MetricsArgs& a, hipStream_t stream);

// Temporal metrics (temporal.hip): backward second and third differences of two point trajectories over ragged sequences,
//   acc[t] = (x[t] - 2 x[t-1] + x[t-2]) fps^2,   jerk[t] = (x[t] - 3 x[t-1] + 3 x[t-2] - x[t-3]) fps^3,
// each defined where all of its frames count (valid != 0) -- never across a frame that does not, never across two rows.
// Per (frame, point): |acc_gt - acc_hat|, |jerk_hat|, |jerk_gt|, float64 from float32 inputs.
constexpr int TEMPORAL_SEGMENT = 32;   // EMPOSE_TEMPORAL_SEGMENT (include/empose_hip.h): frames a lane walks after its lead-in
constexpr int TEMPORAL_DEFINED_ACC = 1, TEMPORAL_DEFINED_JERK = 2;   // bits of `defined`
struct TemporalArgs {
  const float* x_gt; const float* x_hat;   // [N][F][P][3]
  const unsigned char* valid;              // [N][F]
  double* rows;                            // reduce == 0: [N * F][3 P]; reduce == 1: [N * F][6] sums and sums of squares
  unsigned char* defined;                  // [N][F]
  double fps2, fps3;                       // fps^2, fps^3
  int N, F, P, reduce;
};
long temporal_rows_blocks(int N, int F, int P, int reduce);   // workgroups of the launch
hipError_t launch_temporal_rows(const TemporalArgs& a, hipStream_t stream);

// Smoothing of pose sequences (smooth.hip).  A row is [3 J rotation-vector columns | C linear columns | padding]; an *item*
// is one joint or one channel.  Rotations are filtered on SO(3) through unit quaternions, never across a frame that does
// not count (valid == 0; valid == nullptr: every frame counts) and never across two rows.
constexpr int SMOOTH_SEGMENT = 64;      // EMPOSE_SMOOTH_SEGMENT (include/empose_hip.h): frames a workgroup of the window owns
constexpr int SMOOTH_MAX_RADIUS = 32;   // EMPOSE_SMOOTH_MAX_RADIUS
constexpr int SMOOTH_STATE = 6;         // doubles of one-euro state per item: x^ (4; a channel uses the first) | s^ | live
struct SmoothArgs {
  const float* in; float* out;   // [N * F][ld_in], [N * F][ld_out]
  const unsigned char* valid;    // [N][F] or nullptr
  int N, F, J, C, ld_in, ld_out;
  // window: one side of the symmetric kernel, w[0 .. R]
  int R;
  double taps[SMOOTH_MAX_RADIUS + 1];
  // one-euro
  double fps, min_cutoff, beta, d_cutoff;
  const double* state_in; double* state_out;   // [N][J + C][SMOOTH_STATE], each or nullptr
};
long smooth_window_blocks(int N, int F, int J, int C);   // workgroups of the launch
hipError_t launch_smooth_window(const SmoothArgs& a, hipStream_t stream);
hipError_t launch_smooth_one_euro(const SmoothArgs& a, hipStream_t stream);

}  // namespace empose
