// Online training data (include/posendf_amd_online.h): the sampler that draws a pool of noisy poses from a manifold that is resident
// on the device.
//
//   pndf_online_sample_kernel   one lane per joint quaternion of the pool, the shape of pndf_train_batch_kernel: lane e holds joint
//                               j = e - J p of pose p = e / J (64-bit index arithmetic, bounded by count * J).  The lane draws
//                               block 0 of its pose (source row and sigma group: the J lanes of a pose each draw it, nothing
//                               passes between lanes) and block 1 + j (its own four noise words), does one 16-byte load from the
//                               gathered manifold row and one 16-byte store; the lane of joint 0 also writes the pose's row and
//                               group where the caller asked for them.  Consecutive lanes read consecutive 16-byte pieces of a
//                               16 J-byte row and store one contiguous stream.  J is a kernel argument; the instantiation
//                               JC = 21 (pndf_online_sample) divides by the constant instead, as it did when 21 was the only
//                               joint count.
// The arithmetic is pndf_online.h's, shared with the host twin (pndf_cpu.cpp).  The options travel as one kernel argument and
// are read with constant offsets.  Plain vector loads and stores, no LDS, no atomics, no communication between lanes: the same
// (seed, draw, index, options, manifold) give the same bits whatever the launch covers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/posendf_amd_online.h"
#include "../../include/posendf_amd_skeleton_data.h"
#include "pndf_host.h"
#include "pndf_layout.h"
#include "pndf_online.h"

constexpr int PNDF_ONLINE_THREADS = 256;

// JC: the joint count as a constant, or 0 = the argument `joints`
template <int JC>
__global__ void __launch_bounds__(256) pndf_online_sample_kernel(const float4* __restrict__ man_db, long long N, long long first, long long quats,
                                                                 int joints, pndf_online_opts o, float4* __restrict__ q,
                                                                 long long* __restrict__ src, int* __restrict__ group) {
    const int NJ = JC ? JC : joints;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= quats) return;
    const long long p = e / NJ;
    const int j = (int)(e - p * NJ);
    const long long i = first + p;
    int64_t row;
    int32_t g;
    float sigma;
    pndf_online_pick(o, i, N, &row, &g, &sigma);
    float Q[4], u[4];
    pndf_quat_unpack(man_db[row * NJ + j], Q);
    pndf_online_quat(o.seed, o.draw, i, j, o.noise, sigma, Q, u);
    q[e] = make_float4(u[0], u[1], u[2], u[3]);
    if (j == 0) {
        if (src) src[p] = row;
        if (group) group[p] = g;
    }
}

// the stateless entry point has no handle: its refusals go to the slot of a failed pndf_create (pndf_last_error(NULL))
struct pndf_engine;
static int online_fail(int code, const std::string& msg) {
    pndf_null_handle_error<pndf_engine>() = msg;
    return code;
}

// ------------------------------------------------------------------ C ABI (include/posendf_amd_online.h)
// `name`: the entry point, for the texts
static int online_sample(const char* name, const float* man_db, int64_t N, int NJ, int64_t first, int64_t count, const pndf_online_opts* opt,
                         float* q, int64_t* src, int32_t* group, void* stream) {
    PndfRange range(name);
    if (const char* why = pndf_online_check(man_db, N, NJ, first, count, opt, q, src, group, 16))
        return online_fail(PNDF_ERR_BAD_ARG, std::string(name) + ": " + why);
    if (count == 0) return PNDF_OK;
    const PndfDeviceCheck any = pndf_check_gfx950(PNDF_ANY_DEVICE, "the online sampler");
    if (any.code != PNDF_OK) return online_fail(any.code, any.text);
    const int device = pndf_pointer_device(q);
    if (device < 0) return online_fail(PNDF_ERR_BAD_ARG, std::string(name) + ": q is not device memory");
    DeviceGuard guard(device);
    if (!guard.ok) return online_fail(PNDF_ERR_HIP, std::string(name) + ": hipSetDevice failed");
    const long long quats = (long long)count * NJ;
    const unsigned blocks = (unsigned)((quats + PNDF_ONLINE_THREADS - 1) / PNDF_ONLINE_THREADS);
    if (NJ == pndf::NJ)
        hipLaunchKernelGGL(pndf_online_sample_kernel<pndf::NJ>, dim3(blocks), dim3(PNDF_ONLINE_THREADS), 0, (hipStream_t)stream,
                           (const float4*)man_db, (long long)N, (long long)first, quats, NJ, *opt, (float4*)q, (long long*)src, (int*)group);
    else
        hipLaunchKernelGGL(pndf_online_sample_kernel<0>, dim3(blocks), dim3(PNDF_ONLINE_THREADS), 0, (hipStream_t)stream,
                           (const float4*)man_db, (long long)N, (long long)first, quats, NJ, *opt, (float4*)q, (long long*)src, (int*)group);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return online_fail(PNDF_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
    return PNDF_OK;
}

extern "C" int pndf_online_sample(const float* man_db, int64_t N, int64_t first, int64_t count, const pndf_online_opts* opt, float* q,
                                  int64_t* src, int32_t* group, void* stream) {
    return online_sample("pndf_online_sample", man_db, N, pndf::NJ, first, count, opt, q, src, group, stream);
}

// include/posendf_amd_skeleton_data.h
extern "C" int pndf_skel_online_sample(const float* man_db, int64_t N, int32_t num_joints, int64_t first, int64_t count,
                                       const pndf_online_opts* opt, float* q, int64_t* src, int32_t* group, void* stream) {
    return online_sample("pndf_skel_online_sample", man_db, N, num_joints, first, count, opt, q, src, group, stream);
}
