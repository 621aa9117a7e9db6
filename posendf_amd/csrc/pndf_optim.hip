// The two HBM-bound kernels that close a training step around csrc/pndf_train.hip (model/train_posendf.py:92-99,
// model/load_data.py:43-71), so that one step is: batch assembly, pndf_train_forward, pndf_train_backward, optimiser -- with no
// host work, allocation or copy in between.
//   pndf_train_batch_kernel   gathers the step's noisy poses, their labels' mean and the manifold poses out of a data set that
//                             is resident on the device, from raw 32-bit random words: row = off[f] + (word * len_f >> 32).
//                             The joint count is an argument (pndf_skel_train_batch; pndf_train_batch is 21 joints).
//                             One thread per joint quaternion (one 16-byte load, one 16-byte store); the thread of joint 0 of a
//                             noisy pose also reduces the pose's k labels, in index order.
//   pndf_adam_step_kernel     torch.optim.Adam (pndf_adam.h; coupled L2 weight decay, no amsgrad) over ONE flat buffer that holds every
//                             parameter: four 16-byte streams in, three out, no tensor table (the pads between tensors are
//                             zero and stay zero).  Element-wise: the result does not depend on the launch shape.
// Plain vector loads and stores, no atomics, no communication between threads: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/posendf_amd_skeleton_train.h"
#include "pndf_adam.h"
#include "pndf_experiment.h"
#include "pndf_host.h"

PNDF_EXPORT_EXPERIMENT_WORD(optim)

namespace {

constexpr int SMPL_JOINTS = 21;        // pndf_train_batch: joints = 16-byte quaternions per pose
constexpr int MAX_JOINTS = 32;         // pndf_config.parent[32]
constexpr int MAX_BLOCKS = 2048;       // 256 CUs x 8 blocks of 256 threads; the rest of the buffer by grid stride

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pndf_adam_step_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                        float* __restrict__ m, float* __restrict__ v,
                                                                        long long n, AdamScalars s) {
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 P = reinterpret_cast<float4*>(p)[i];
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        float4 M = reinterpret_cast<float4*>(m)[i];
        float4 V = reinterpret_cast<float4*>(v)[i];
        adam_one(P.x, G.x, M.x, V.x, s);
        adam_one(P.y, G.y, M.y, V.y, s);
        adam_one(P.z, G.z, M.z, V.z, s);
        adam_one(P.w, G.w, M.w, V.w, s);
        reinterpret_cast<float4*>(p)[i] = P;
        reinterpret_cast<float4*>(m)[i] = M;
        reinterpret_cast<float4*>(v)[i] = V;
    }
    // the tail of a buffer whose length is not a multiple of four: at most three elements, the first threads of block 0
    const long long t = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) {
        float P = p[t], M = m[t], V = v[t];
        adam_one(P, g[t], M, V, s);
        p[t] = P;
        m[t] = M;
        v[t] = V;
    }
}

struct BatchArgs {
    const float4* pose_db;
    const float* dist_db;
    const float4* man_db;
    const long long* file_off;
    const long long* man_off;
    const int* item_file;
    const int* item_man_file;
    const unsigned* words;
    float4* q;
    float* dist_gt;
    float4* q_man;
    long long quats;          // items * num_pts * nj: 16-byte elements per side
    int F, Fm, k, num_pts, flip, nj;
};

// Grid: the noisy side's quaternions, then the manifold side's.  A file index outside the table or an empty file cannot be
// sampled: such a pose is written as NaN and nothing is read (the host refuses both before it launches what it can see).
extern "C" __global__ void __launch_bounds__(256) pndf_train_batch_kernel(BatchArgs a) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= 2 * a.quats) return;
    const int side = id >= a.quats;
    const long long e = side ? id - a.quats : id;
    const long long pose = e / a.nj;
    const int j = (int)(e - pose * a.nj);
    const long long item = pose / a.num_pts;
    const int i = (int)(pose - item * a.num_pts);
    const int f = side ? a.item_man_file[item] : a.item_file[item];
    const int nf = side ? a.Fm : a.F;
    const long long* off = side ? a.man_off : a.file_off;
    float4* out = side ? a.q_man : a.q;
    long long len = 0, first = 0;
    if (f >= 0 && f < nf) {
        first = off[f];
        len = off[f + 1] - first;
    }
    if (len <= 0 || len > 0xffffffffll) {
        const float nan = __builtin_nanf("");
        out[e] = make_float4(nan, nan, nan, nan);
        if (!side && j == 0) a.dist_gt[pose] = nan;
        return;
    }
    const unsigned w = a.words[(item * 2 + side) * a.num_pts + i];
    const long long row = first + (long long)(((unsigned long long)w * (unsigned long long)len) >> 32);
    float4 x = (side ? a.man_db : a.pose_db)[row * a.nj + j];
    if (a.flip && x.x < 0.0f) x = make_float4(-x.x, -x.y, -x.z, -x.w);     // quat_flip, load_data.py:12-16
    out[e] = x;
    if (!side && j == 0) {
        const float* d = a.dist_db + row * a.k;
        float acc = d[0];
        for (int c = 1; c < a.k; ++c) acc += d[c];
        a.dist_gt[pose] = acc / (float)a.k;                                  // np.mean(dist, axis=1), load_data.py:53
    }
}

// ------------------------------------------------------------------ C ABI (include/posendf_amd.h)
extern "C" int pndf_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1,
                              double beta2, double eps, double weight_decay, void* stream) {
    PndfRange range("pndf_adam_step");
    if (n < 0 || step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return PNDF_ERR_BAD_ARG;
    if (n == 0) return PNDF_OK;
    if (!p || !g || !m || !v) return PNDF_ERR_BAD_ARG;
    if ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) return PNDF_ERR_BAD_ARG;
    DeviceGuard guard(pndf_pointer_device(p));
    if (!guard.ok) return PNDF_ERR_HIP;
    const AdamScalars s = pndf_adam_scalars(step, lr, beta1, beta2, eps, weight_decay);      // as torch forms them (pndf_adam.h)
    const long long n4 = (long long)(n >> 2);
    long long blocks = (n4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    hipLaunchKernelGGL(pndf_adam_step_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long long)n, s);
    return hipGetLastError() == hipSuccess ? PNDF_OK : PNDF_ERR_HIP;
}

extern "C" int pndf_skel_train_batch(const float* pose_db, const float* dist_db, const float* man_db, const int64_t* file_off,
                                     const int64_t* man_off, const int32_t* item_file, const int32_t* item_man_file,
                                     const uint32_t* words, int32_t F, int32_t Fm, int32_t k, int32_t items, int32_t num_pts,
                                     int32_t flip, int32_t num_joints, float* q, float* dist_gt, float* q_man, void* stream) {
    PndfRange range("pndf_train_batch");
    if (num_joints < 1 || num_joints > MAX_JOINTS) return PNDF_ERR_BAD_ARG;
    if (F < 1 || Fm < 1 || k < 1 || items < 0 || num_pts < 0) return PNDF_ERR_BAD_ARG;
    if (items == 0 || num_pts == 0) return PNDF_OK;
    if (!pose_db || !dist_db || !man_db || !file_off || !man_off || !item_file || !item_man_file || !words || !q || !dist_gt || !q_man)
        return PNDF_ERR_BAD_ARG;
    if ((((uintptr_t)pose_db) | ((uintptr_t)man_db) | ((uintptr_t)q) | ((uintptr_t)q_man) | ((uintptr_t)dist_gt)) & 15) return PNDF_ERR_BAD_ARG;
    if ((((uintptr_t)file_off) | ((uintptr_t)man_off)) & 7) return PNDF_ERR_BAD_ARG;
    if ((((uintptr_t)dist_db) | ((uintptr_t)item_file) | ((uintptr_t)item_man_file) | ((uintptr_t)words)) & 3) return PNDF_ERR_BAD_ARG;
    const long long quats = (long long)items * num_pts * num_joints;
    const long long blocks = (2 * quats + 255) / 256;
    if (blocks > 0x7fffffffll) return PNDF_ERR_BAD_ARG;
    DeviceGuard guard(pndf_pointer_device(q));
    if (!guard.ok) return PNDF_ERR_HIP;
    BatchArgs a;
    a.pose_db = reinterpret_cast<const float4*>(pose_db);
    a.dist_db = dist_db;
    a.man_db = reinterpret_cast<const float4*>(man_db);
    a.file_off = reinterpret_cast<const long long*>(file_off);
    a.man_off = reinterpret_cast<const long long*>(man_off);
    a.item_file = item_file;
    a.item_man_file = item_man_file;
    a.words = words;
    a.q = reinterpret_cast<float4*>(q);
    a.dist_gt = dist_gt;
    a.q_man = reinterpret_cast<float4*>(q_man);
    a.quats = quats;
    a.F = F; a.Fm = Fm; a.k = k; a.num_pts = num_pts; a.flip = flip ? 1 : 0; a.nj = num_joints;
    hipLaunchKernelGGL(pndf_train_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PNDF_OK : PNDF_ERR_HIP;
}

extern "C" int pndf_train_batch(const float* pose_db, const float* dist_db, const float* man_db, const int64_t* file_off,
                                const int64_t* man_off, const int32_t* item_file, const int32_t* item_man_file,
                                const uint32_t* words, int32_t F, int32_t Fm, int32_t k, int32_t items, int32_t num_pts,
                                int32_t flip, float* q, float* dist_gt, float* q_man, void* stream) {
    return pndf_skel_train_batch(pose_db, dist_db, man_db, file_off, man_off, item_file, item_man_file, words, F, Fm, k, items, num_pts,
                                 flip, SMPL_JOINTS, q, dist_gt, q_man, stream);
}
