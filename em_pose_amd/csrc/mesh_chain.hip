// Full mesh (final vertices): the kinematic chain to relative bone transforms and joints, and its reverse.  The dense
// skinning of all V vertices is mesh_rows.hip's mesh_rows_kernel (mesh_x3.hip by default), its reverse mesh_vjp.hip.
#include "mesh_kernels.h"
#include "smpl_kernels.h"

namespace empose {

__global__ void mesh_chain_kernel(MeshChainArgs a) {
  // one thread per (frame, joint): walks from the root down to its joint with the running transform (3 x 3 | t) in
  // registers.  (Round 6: a thread per (frame, joint, ROW) before -- three times the threads, each repeating the walk and
  // the ancestor look-ups for one row: 119 us per 16384 frames, a tenth of the full-mesh evaluation.)  Joints >= NB (the 30
  // hand joints of SMPL-H) have zero pose on this path (reference smpl.py:99), i.e. identity rotation under either
  // Rodrigues convention: they only translate along their parent's frame and get no skinning transform of their own
  // (weights folded into the wrists).
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int nj = a.n_joints;
  // (the parent table in LDS: the walks below are chains of dependent look-ups, ~80 per thread)
  __shared__ int parents_s[MESH_MAX_JOINTS];
  for (int i = threadIdx.x; i < nj; i += blockDim.x) parents_s[i] = a.parents[i];
  __syncthreads();
  if (idx >= a.T * nj) return;
  const int t = idx / nj, j = idx % nj;
  const float* R = a.rot + (size_t)t * NB * 9;
  const float* J = a.out + (size_t)t * a.ncp + a.j_off;
  // the joints from the root down to j, without a per-thread array of the path (a dynamically indexed array lives in
  // scratch memory): the ancestor k levels above j is found by walking up k times -- chains are at most a dozen joints long
  int n = 0;
  for (int q = j; q >= 0; q = parents_s[q]) ++n;
  float G[3][3], tr[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    G[r][0] = R[r * 3 + 0]; G[r][1] = R[r * 3 + 1]; G[r][2] = R[r * 3 + 2];
    tr[r] = J[r];
  }
  int prev = 0;
  for (int k = n - 2; k >= 0; --k) {
    int q = j;
    for (int up = 0; up < k; ++up) q = parents_s[q];
    const float* Jq = J + q * 3;
    const float* Jp = J + prev * 3;
    const float dx = Jq[0] - Jp[0], dy = Jq[1] - Jp[1], dz = Jq[2] - Jp[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) tr[r] = G[r][0] * dx + G[r][1] * dy + G[r][2] * dz + tr[r];
    if (q < NB) {
      const float* Rq = R + q * 9;
      float Rv[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) Rv[e] = Rq[e];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float n0 = G[r][0] * Rv[0] + G[r][1] * Rv[3] + G[r][2] * Rv[6];
        const float n1 = G[r][0] * Rv[1] + G[r][1] * Rv[4] + G[r][2] * Rv[7];
        const float n2 = G[r][0] * Rv[2] + G[r][1] * Rv[5] + G[r][2] * Rv[8];
        G[r][0] = n0; G[r][1] = n1; G[r][2] = n2;
      }
    }
    prev = q;
  }
  if (j < NB) {
    const float* Jj = J + j * 3;
    // relative transform, row r: (G^R[r][0..2], A^t[r]) -- one 16-byte read per (bone, row) in the skinning epilogue
#pragma unroll
    for (int r = 0; r < 3; ++r)
      *reinterpret_cast<float4*>(a.xf + (((size_t)t * NB + j) * 3 + r) * 4) =
          make_float4(G[r][0], G[r][1], G[r][2], tr[r] - (G[r][0] * Jj[0] + G[r][1] * Jj[1] + G[r][2] * Jj[2]));
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
    a.joints[(size_t)t * nj * 3 + j * 3 + r] = tr[r] + (a.trans ? a.trans[(size_t)t * 3 + r] : 0.f);
}

hipError_t launch_mesh_chain(const MeshChainArgs& a, hipStream_t stream) {
  const long n = (long)a.T * a.n_joints;
  hipLaunchKernelGGL(mesh_chain_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---- the transforms in float64 (mesh_kernels.h MeshChainF64Args) -----------------------------------------------------
// One thread per (frame, body joint): Rodrigues in double, both conventions as smpl_math.h states them.
__global__ void mesh_rot_f64_kernel(MeshChainF64Args a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.T * NB) return;
  const float* th = a.poses + (size_t)(idx / NB) * 66 + (idx % NB) * 3;
  const double rx = th[0], ry = th[1], rz = th[2];
  double ang;
  if (a.rod_conv == 0) {
    const double ux = rx + 1e-8, uy = ry + 1e-8, uz = rz + 1e-8;
    ang = sqrt(ux * ux + uy * uy + uz * uz);
  } else {
    ang = sqrt(fmax(rx * rx + ry * ry + rz * rz, 1e-4));
  }
  const double dx = rx / ang, dy = ry / ang, dz = rz / ang, s = sin(ang), oc = 1.0 - cos(ang);
  double* R = a.rot + (size_t)idx * 9;
  R[0] = 1.0 + oc * (-dz * dz - dy * dy); R[1] = -s * dz + oc * (dx * dy);        R[2] = s * dy + oc * (dx * dz);
  R[3] = s * dz + oc * (dx * dy);         R[4] = 1.0 + oc * (-dz * dz - dx * dx); R[5] = -s * dx + oc * (dy * dz);
  R[6] = -s * dy + oc * (dx * dz);        R[7] = s * dx + oc * (dy * dz);         R[8] = 1.0 + oc * (-dy * dy - dx * dx);
}

// One thread per (frame, rest-joint coordinate): the row of wc times the feature row [vec(R_j - I), j = 1..21 | beta | 1].
__global__ void mesh_jrest_f64_kernel(MeshChainF64Args a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.T * NB * 3) return;
  const int t = idx / (NB * 3), c = idx % (NB * 3);
  const float* __restrict__ w = a.wj + (size_t)c * 200;
  const double* __restrict__ R = a.rot + (size_t)t * NB * 9 + 9;
  double s = w[199];
  for (int k = 0; k < 189; ++k) s += (double)w[k] * (R[k] - ((k % 9) % 4 == 0 ? 1.0 : 0.0));
  for (int k = 0; k < 10; ++k) s += (double)w[189 + k] * (double)a.betas[(size_t)t * 10 + k];
  a.jrest[idx] = s;
}

// mesh_chain_kernel in double for the body joints, transforms only.
__global__ void mesh_chain_f64_kernel(MeshChainF64Args a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  __shared__ int parents_s[NB];
  for (int i = threadIdx.x; i < NB; i += blockDim.x) parents_s[i] = a.parents[i];
  __syncthreads();
  if (idx >= a.T * NB) return;
  const int t = idx / NB, j = idx % NB;
  const double* R = a.rot + (size_t)t * NB * 9;
  const double* J = a.jrest + (size_t)t * NB * 3;
  int n = 0;
  for (int q = j; q >= 0; q = parents_s[q]) ++n;
  double G[3][3], tr[3];
  for (int r = 0; r < 3; ++r) {
    G[r][0] = R[r * 3 + 0]; G[r][1] = R[r * 3 + 1]; G[r][2] = R[r * 3 + 2];
    tr[r] = J[r];
  }
  int prev = 0;
  for (int k = n - 2; k >= 0; --k) {
    int q = j;
    for (int up = 0; up < k; ++up) q = parents_s[q];
    const double dx = J[q * 3] - J[prev * 3], dy = J[q * 3 + 1] - J[prev * 3 + 1], dz = J[q * 3 + 2] - J[prev * 3 + 2];
    for (int r = 0; r < 3; ++r) tr[r] = G[r][0] * dx + G[r][1] * dy + G[r][2] * dz + tr[r];
    const double* Rv = R + q * 9;
    for (int r = 0; r < 3; ++r) {
      const double n0 = G[r][0] * Rv[0] + G[r][1] * Rv[3] + G[r][2] * Rv[6];
      const double n1 = G[r][0] * Rv[1] + G[r][1] * Rv[4] + G[r][2] * Rv[7];
      const double n2 = G[r][0] * Rv[2] + G[r][1] * Rv[5] + G[r][2] * Rv[8];
      G[r][0] = n0; G[r][1] = n1; G[r][2] = n2;
    }
    prev = q;
  }
  const double* Jj = J + j * 3;
  for (int r = 0; r < 3; ++r)
    *reinterpret_cast<float4*>(a.xf + (((size_t)t * NB + j) * 3 + r) * 4) =
        make_float4((float)G[r][0], (float)G[r][1], (float)G[r][2],
                    (float)(tr[r] - (G[r][0] * Jj[0] + G[r][1] * Jj[1] + G[r][2] * Jj[2])));
}

hipError_t launch_mesh_chain_f64(const MeshChainF64Args& a, hipStream_t stream) {
  if (a.T <= 0) return hipErrorInvalidValue;
  const long n = (long)a.T * NB;
  hipLaunchKernelGGL(mesh_rot_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(mesh_jrest_f64_kernel, dim3((unsigned)((n * 3 + 255) / 256)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(mesh_chain_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// Reverse of mesh_chain_kernel (+ the skinning transforms): one thread per frame.  Forward, per joint j with parent p:
// G_j = G_p R_j (R_j = I for the hand joints), t_j = G_p (J_j - J_p) + t_p, joints_j = t_j + trans, and per body bone
// A_b = [G_b | t_b - G_b J_b].  The joints are visited from the last to the root, so that dt_j and dG_j are complete when
// j is reached (children have larger ids):
//   dR_j = G_p^T dG_j,   dG_p += dG_j R_j^T + dt_j (J_j - J_p)^T,   dt_p += dt_j,
//   dJ_j = G_p^T dt_j - G_j^T (dt_j - dJoint_j)   (the children's share -G_j^T sum_c dt_c and dA's -G_j^T dA^t_j in one)
// with dG_j = dA_j^R - dA_j^t J_j^T and dt_j = dJoint_j + dA_j^t to begin with.  A hand joint's G is its body
// ancestor's, so its dG goes straight there.  Per-frame state in LDS as [item][frame]: 22 G, 22 dG, 52 dt.
constexpr int MCB_FR = 16;   // frames per block: 35 KB of LDS
__global__ __launch_bounds__(MCB_FR) void mesh_chain_bwd_kernel(MeshChainBwdArgs a) {
  __shared__ float G_s[NB * 9][MCB_FR];
  __shared__ float dG_s[NB * 9][MCB_FR];
  __shared__ float dt_s[MESH_MAX_JOINTS * 3][MCB_FR];
  __shared__ int parents_s[MESH_MAX_JOINTS], body_s[MESH_MAX_JOINTS];
  const int nj = a.n_joints;
  if (threadIdx.x == 0)
    for (int j = 0; j < nj; ++j) {
      parents_s[j] = a.parents[j];
      body_s[j] = j < NB ? j : body_s[a.parents[j]];   // nearest body ancestor (parents come first)
    }
  __syncthreads();
  const int t = blockIdx.x * MCB_FR + threadIdx.x;
  if (t >= a.T) return;
  const int f = threadIdx.x;
  const float* R = a.rot + (size_t)t * NB * 9;
  const float* J = a.jrest + (size_t)t * a.ld_j;
  // global rotations of the body joints
  for (int j = 0; j < NB; ++j) {
    const float* Rj = R + j * 9;
    if (j == 0) {
      for (int e = 0; e < 9; ++e) G_s[e][f] = Rj[e];
      continue;
    }
    const int p = parents_s[j];
    float Gp[9];
    for (int e = 0; e < 9; ++e) Gp[e] = G_s[p * 9 + e][f];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        G_s[j * 9 + r * 3 + c][f] = Gp[r * 3] * Rj[c] + Gp[r * 3 + 1] * Rj[3 + c] + Gp[r * 3 + 2] * Rj[6 + c];
  }
  const float* dA = a.dA ? a.dA + (size_t)t * MESH_VJP_DA : nullptr;
  const float* dJ = a.dJ ? a.dJ + (size_t)t * nj * 3 : nullptr;
  for (int j = 0; j < nj; ++j)
    for (int r = 0; r < 3; ++r)
      dt_s[j * 3 + r][f] = (dJ ? dJ[j * 3 + r] : 0.f) + (dA && j < NB ? dA[j * 12 + r * 4 + 3] : 0.f);
  for (int j = 0; j < NB; ++j)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        dG_s[j * 9 + r * 3 + c][f] = dA ? dA[j * 12 + r * 4 + c] - dA[j * 12 + r * 4 + 3] * J[j * 3 + c] : 0.f;
  float* dR = a.d_rot + (size_t)t * NB * 9;
  float* dJr = a.d_jrest + (size_t)t * a.ld_dj;
  for (int j = nj - 1; j >= 0; --j) {
    const int bj = body_s[j];
    float Gj[9], dt[3], dtx[3];
    for (int e = 0; e < 9; ++e) Gj[e] = G_s[bj * 9 + e][f];
    for (int r = 0; r < 3; ++r) {
      dt[r] = dt_s[j * 3 + r][f];
      dtx[r] = dt[r] - (dJ ? dJ[j * 3 + r] : 0.f);   // sum_c dt_c + dA^t_j
    }
    if (j == 0) {
      for (int c = 0; c < 3; ++c) {
        dJr[c] = dt[c] - (Gj[c] * dtx[0] + Gj[3 + c] * dtx[1] + Gj[6 + c] * dtx[2]);
        for (int r = 0; r < 3; ++r) dR[r * 3 + c] = dG_s[r * 3 + c][f];
      }
      break;
    }
    const int p = parents_s[j], bp = body_s[p];
    float Gp[9];
    for (int e = 0; e < 9; ++e) Gp[e] = G_s[bp * 9 + e][f];
    for (int c = 0; c < 3; ++c)
      dJr[j * 3 + c] = (Gp[c] * dt[0] + Gp[3 + c] * dt[1] + Gp[6 + c] * dt[2]) -
                       (Gj[c] * dtx[0] + Gj[3 + c] * dtx[1] + Gj[6 + c] * dtx[2]);
    for (int r = 0; r < 3; ++r) dt_s[p * 3 + r][f] += dt[r];
    const float rel[3] = {J[j * 3] - J[p * 3], J[j * 3 + 1] - J[p * 3 + 1], J[j * 3 + 2] - J[p * 3 + 2]};
    float dGp[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) dGp[r * 3 + c] = dt[r] * rel[c];
    if (j < NB) {
      const float* Rj = R + j * 9;
      float dGj[9];
      for (int e = 0; e < 9; ++e) dGj[e] = dG_s[j * 9 + e][f];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          dR[j * 9 + r * 3 + c] = Gp[r] * dGj[c] + Gp[3 + r] * dGj[3 + c] + Gp[6 + r] * dGj[6 + c];   // G_p^T dG_j
          dGp[r * 3 + c] += dGj[r * 3] * Rj[c * 3] + dGj[r * 3 + 1] * Rj[c * 3 + 1] + dGj[r * 3 + 2] * Rj[c * 3 + 2];
        }
    }
    for (int e = 0; e < 9; ++e) dG_s[bp * 9 + e][f] += dGp[e];
  }
  for (int c = nj * 3; c < a.ld_dj; ++c) dJr[c] = 0.f;
  if (a.g_trans)   // sum_v dV_v (the feat sweep's slices, double) + sum_j dJoint_j, rounded once
    for (int r = 0; r < 3; ++r) {
      double s = 0.0;
      for (int k = 0; a.dtrans && k < a.n_slices; ++k) s += a.dtrans[((size_t)k * a.T + t) * 3 + r];
      for (int j = 0; dJ && j < nj; ++j) s += dJ[j * 3 + r];
      a.g_trans[(size_t)t * 3 + r] = (float)s;
    }
}

hipError_t launch_mesh_chain_bwd(const MeshChainBwdArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(mesh_chain_bwd_kernel, dim3((unsigned)((a.T + MCB_FR - 1) / MCB_FR)), dim3(MCB_FR), 0, stream, a);
  return hipGetLastError();
}

}  // namespace empose
