// Stand-alone host program (own main, no HIP, no library): the host twin's moving-camera path -- pndf_project_ex_cpu with a
// pndf_project_options10 (include/posendf_amd.h, pndf_fk_cams_energy_grad of csrc/pndf_fk.h) -- on a 15-joint hand with synthetic weights,
// three tracks of T = 5 frames, K = 20 keypoints (the joints and a tip on every leaf) seen by V = 2 cameras whose table is given per pose
// [B,V,16] or per frame [T,V,16], a free root per pose coupled to its neighbour frames'.  Every buffer is exactly as long as the call reads
// it: a block read behind the per-frame table (an index that forgot the modulus) is one past an allocation.  Built with csrc/pndf_cpu.cpp
// in the same command; meant for a sanitizer build on the CPU,
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -pthread tests/host/skeleton_cams_check.cpp
//         posendf_amd/csrc/pndf_cpu.cpp -o skeleton_cams_check
// and checked without one by tests/test_skeleton_cams_host.py.  Exit status 0 and one line that names what was checked.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/posendf_amd.h"

namespace {

const int32_t HAND[15] = {-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13};
constexpr int J = 15, NQ = 4 * J, P = 3, T = 5, B = P * T, K = J + 5, V = 2;
constexpr float LAM_ROT = 0.375f, LAM_TRANS = 0.25f, NU_ROT = 0.05f, NU_TRANS = 0.1f;

uint32_t rng_state = 24680u;
float uniform() {      // [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        printf("skeleton_cams_check: FAILED %s\n", what);
        ++failures;
    }
}

bool same_bits(const float* a, const float* b, size_t n) { return memcmp(a, b, n * sizeof(float)) == 0; }

// row v of a rig turned by `angle` about y and moved by `shift` along x: fx fy cx cy, R [9], t [3]
void view_row(float* row, int v, float angle, float shift) {
    const float a = angle + 0.4f * (float)v, c = cosf(a), s = sinf(a);
    const float R[9] = {c, 0.f, -s, 0.f, 1.f, 0.f, s, 0.f, c};
    row[0] = 500.f + 10.f * (float)v; row[1] = 480.f; row[2] = 320.f; row[3] = 240.f;
    for (int i = 0; i < 9; ++i) row[4 + i] = R[i];
    row[13] = -shift - 0.12f * (float)v; row[14] = 0.f; row[15] = 5.f * (1.f - c);
}

}  // namespace

int main() {
    pndf_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.act = 1;      // lrelu
    cfg.beta = 100.0f;
    cfg.num_joints = J;
    const int32_t dims[4] = {6 * J, 24, 16, 1};
    cfg.n_dims = 4;
    for (int i = 0; i < 4; ++i) cfg.dims[i] = dims[i];
    for (int j = 0; j < J; ++j) cfg.parent[j] = HAND[j];
    cfg.precision = PNDF_PREC_FP32;
    cfg.enc_act = -1;
    pndf_cpu_handle h = nullptr;
    if (pndf_cpu_create(&h, &cfg) != 0) {
        printf("skeleton_cams_check: pndf_cpu_create failed: %s\n", pndf_cpu_last_error(nullptr));
        return 1;
    }
    std::vector<std::vector<float>> tensors;
    auto tensor = [&](int64_t n, float scale, float shift) {
        std::vector<float> t((size_t)n);
        for (float& x : t) x = (uniform() - 0.5f) * scale + shift;
        tensors.push_back(t);
    };
    for (int j = 0; j < J; ++j) {
        const int in = HAND[j] < 0 ? 4 : 10;
        tensor(10 * in, 2.0f / sqrtf((float)in), 0.f);
        tensor(10, 0.2f, 0.f);
        tensor(6 * 10, 2.0f / sqrtf(10.f), 0.f);
        tensor(6, 0.2f, 0.f);
    }
    for (int l = 0; l < 3; ++l) {
        tensor((int64_t)dims[l + 1] * dims[l], 4.0f / sqrtf((float)dims[l]), 0.f);
        tensor(dims[l + 1], 0.2f, l == 2 ? 0.3f : 0.f);
    }
    std::vector<const float*> ptrs;
    std::vector<int64_t> numel;
    for (const auto& t : tensors) {
        ptrs.push_back(t.data());
        numel.push_back((int64_t)t.size());
    }
    if (pndf_cpu_load_weights(h, ptrs.data(), numel.data(), (int)ptrs.size()) != 0) {
        printf("skeleton_cams_check: pndf_cpu_load_weights failed: %s\n", pndf_cpu_last_error(h));
        return 1;
    }
    std::vector<float> q((size_t)B * NQ);
    for (int i = 0; i < B * J; ++i) {
        float v[4], n = 0.f;
        for (float& x : v) {
            x = uniform() - 0.5f;
            n += x * x;
        }
        for (int c = 0; c < 4; ++c) q[(size_t)i * 4 + c] = v[c] / sqrtf(n);
    }
    std::vector<float> rest((size_t)J * 3), offset((size_t)K * 3, 0.f);
    std::vector<int32_t> joint((size_t)K);
    for (float& x : rest) x = 1.5f * (uniform() - 0.5f);
    for (int k = 0; k < K; ++k) joint[(size_t)k] = k < J ? k : 3 * (k - J) + 2;
    for (int i = 3 * J; i < 3 * K; ++i) offset[(size_t)i] = uniform() - 0.5f;
    std::vector<float> target((size_t)B * V * K * 2), conf((size_t)B * V * K);
    for (int i = 0; i < B * V * K; ++i) {
        target[(size_t)i * 2] = 320.f + 150.f * (uniform() - 0.5f);
        target[(size_t)i * 2 + 1] = 240.f + 150.f * (uniform() - 0.5f);
        conf[(size_t)i] = 0.25f + 0.75f * uniform();
    }
    std::vector<float> root0((size_t)B * 7);
    for (int f = 0; f < B; ++f) {
        float* r = &root0[(size_t)f * 7];
        r[0] = 1.5f;
        for (int c = 1; c < 4; ++c) r[c] = 0.3f * (uniform() - 0.5f);
        r[4] = 0.5f * (uniform() - 0.5f);
        r[5] = 0.5f * (uniform() - 0.5f);
        r[6] = 5.f + 0.5f * (uniform() - 0.5f);
    }
    // the tables: one static [V,16]; a path [T,V,16] (the rig turns and moves with the frame); the path repeated for every track [B,V,16];
    // the static table repeated for every pose
    std::vector<float> fixed((size_t)V * 16), path((size_t)T * V * 16), tiled((size_t)B * V * 16), fixed_tiled((size_t)B * V * 16);
    for (int v = 0; v < V; ++v) view_row(&fixed[(size_t)v * 16], v, 0.f, 0.f);
    for (int k = 0; k < T; ++k)
        for (int v = 0; v < V; ++v) view_row(&path[(size_t)(k * V + v) * 16], v, 0.05f * (float)k, 0.1f * (float)k);
    for (int f = 0; f < B; ++f) {
        memcpy(&tiled[(size_t)f * V * 16], &path[(size_t)(f % T) * V * 16], sizeof(float) * V * 16);
        memcpy(&fixed_tiled[(size_t)f * V * 16], fixed.data(), sizeof(float) * V * 16);
    }

    // one call: `steps` steps from `start` with roots `rt` (in place).  kind 0: the 256-byte struct with the static table `tb`; 1: the
    // 280-byte struct with `tb` per pose; 2: with `tb` per frame
    struct Result {
        std::vector<float> out, d, energy, root;
        int rc;
    };
    auto call = [&](const std::vector<float>& start, const std::vector<float>& rt, int steps, int kind, const float* tb, const std::vector<float>& tg,
                    const std::vector<float>& cf, float lam_rot, float lam_trans, uint32_t flags = 0u, int n_views = V) {
        Result r{std::vector<float>((size_t)B * NQ, 7.0f), std::vector<float>((size_t)B, 7.0f), std::vector<float>((size_t)B, 7.0f), rt, 0};
        pndf_project_options10 o;
        memset(&o, 0, sizeof o);
        pndf_project_options8& o8 = o.base9.base8;
        pndf_project_options6& o6 = o8.base7.base6;
        pndf_project_options5& o5 = o6.base5;
        pndf_project_options& base = o5.base4.base3.base2.base;
        base.struct_size = kind == 0 ? sizeof(pndf_project_options9) : sizeof o;      // (pndf_default_project_options lives in the device library)
        base.step_size = 1.0f;
        base.renorm = PNDF_RENORM_UNIT;
        o5.base4.base3.frames = T;
        o5.base4.base3.lambda = 0.5f;
        o5.base4.base3.fill = PNDF_TRACK_GIVEN;
        o5.base4.flags = PNDF_TRACK_FREE_ENDS;
        o5.kp_target = tg.data();
        o5.kp_conf = cf.data();
        o5.kp_energy = r.energy.data();
        o5.rest = rest.data();
        o5.kp_joint = joint.data();
        o5.kp_offset = offset.data();
        o5.n_keypoints = K;
        o5.nu = 0.1f;
        o6.root = r.root.data();
        o6.rho = 0.25f;
        o6.nu_rot = NU_ROT;
        o6.nu_trans = NU_TRANS;
        o6.kp_flags = PNDF_KP_IMAGE;
        o.base9.lambda_rot = lam_rot;
        o.base9.lambda_trans = lam_trans;
        if (kind == 0) {
            o8.views = tb;
            o8.n_views = V;
        } else {
            o.pose_views = tb;
            o.n_pose_views = n_views;
            o.view_flags = flags | (kind == 2 ? (uint32_t)PNDF_VIEWS_PER_FRAME : 0u);
        }
        r.rc = pndf_project_ex_cpu(h, start.data(), r.out.data(), r.d.data(), B, steps, (const pndf_project_options*)&o);
        return r;
    };
    auto same = [&](const Result& a, const Result& b) {
        return a.rc == 0 && b.rc == 0 && same_bits(a.out.data(), b.out.data(), a.out.size()) && same_bits(a.d.data(), b.d.data(), a.d.size()) &&
               same_bits(a.energy.data(), b.energy.data(), a.energy.size()) && same_bits(a.root.data(), b.root.data(), a.root.size());
    };

    // 1. the reduction: every block equal to one table is the call with that static table, bit for bit -- per pose and per frame, the root in
    //    place (no coupling) and out of place (coupled), 0 .. 3 steps
    for (int coupled = 0; coupled < 2; ++coupled)
        for (int steps = 0; steps <= 3; ++steps) {
            const float lr = coupled ? LAM_ROT : 0.f, lt = coupled ? LAM_TRANS : 0.f;
            const Result st = call(q, root0, steps, 0, fixed.data(), target, conf, lr, lt);
            expect(st.rc == 0, "the static call runs");
            expect(same(call(q, root0, steps, 1, fixed_tiled.data(), target, conf, lr, lt), st), "equal blocks per pose are the static call");
            std::vector<float> per_frame((size_t)T * V * 16);
            memcpy(per_frame.data(), fixed_tiled.data(), sizeof(float) * per_frame.size());
            expect(same(call(q, root0, steps, 2, per_frame.data(), target, conf, lr, lt), st), "equal blocks per frame are the static call");
        }

    // 2. a moving rig: finite, moved; the table per frame is the table per pose with the path repeated for every track; `steps` steps are
    //    `steps` chained one-step calls bit for bit (both parities of the root buffer)
    const Result three = call(q, root0, 3, 1, tiled.data(), target, conf, LAM_ROT, LAM_TRANS);
    expect(three.rc == 0, "three steps with a table per pose run");
    if (three.rc != 0) printf("skeleton_cams_check: %s\n", pndf_cpu_last_error(h));
    for (int f = 0; f < B; ++f) {
        const float* r = &three.root[(size_t)f * 7];
        bool finite = true;
        for (int i = 0; i < 7; ++i) finite = finite && isfinite(r[i]);
        expect(finite, "a root under a moving rig is finite");
        expect(!same_bits(r, &root0[(size_t)f * 7], 7), "a root under a moving rig has moved");
        expect(three.energy[(size_t)f] > 0.f, "a pose under a moving rig has energy");
    }
    expect(same(call(q, root0, 3, 2, path.data(), target, conf, LAM_ROT, LAM_TRANS), three), "the table per frame is the path repeated per track");
    expect(!same(call(q, root0, 3, 1, fixed_tiled.data(), target, conf, LAM_ROT, LAM_TRANS), three), "the moving rig differs from the static one");
    for (int kind = 1; kind <= 2; ++kind) {
        const float* tb = kind == 1 ? tiled.data() : path.data();
        Result chain = call(q, root0, 1, kind, tb, target, conf, LAM_ROT, LAM_TRANS);
        const Result two = call(q, root0, 2, kind, tb, target, conf, LAM_ROT, LAM_TRANS);
        chain = call(chain.out, chain.root, 1, kind, tb, target, conf, LAM_ROT, LAM_TRANS);
        expect(same(chain, two), "two steps are two chained one-step calls");
        chain = call(chain.out, chain.root, 1, kind, tb, target, conf, LAM_ROT, LAM_TRANS);
        expect(same(chain, three), "three steps are three chained one-step calls");
    }

    // 3. the skip: a row whose fx is 0, whose fy is NaN, and a row of zeros switch their view off for that pose before anything of it is read
    //    (its targets and confidences hold NaN): the call with valid rows and zero confidences there, bit for bit, and nothing is NaN
    {
        std::vector<float> bad = tiled, off = conf, nan_conf = conf, nan_target = target;
        const int poses[3] = {1, 7, 13}, views[3] = {0, 1, 0};
        for (int i = 0; i < 3; ++i) {
            float* row = &bad[(size_t)(poses[i] * V + views[i]) * 16];
            if (i == 0) row[0] = 0.f;
            if (i == 1) row[1] = NAN;
            if (i == 2) memset(row, 0, sizeof(float) * 16);
            for (int k = 0; k < K; ++k) {
                const size_t at = (size_t)(poses[i] * V + views[i]) * K + k;
                off[at] = 0.f;
                nan_conf[at] = NAN;
                nan_target[2 * at] = nan_target[2 * at + 1] = NAN;
            }
        }
        const Result want = call(q, root0, 3, 1, tiled.data(), target, off, LAM_ROT, LAM_TRANS);
        const Result got = call(q, root0, 3, 1, bad.data(), nan_target, nan_conf, LAM_ROT, LAM_TRANS);
        expect(same(got, want), "a view without a positive focal length is a view with zero confidences");
        bool finite = got.rc == 0;
        for (float x : got.out) finite = finite && isfinite(x);
        for (float x : got.root) finite = finite && isfinite(x);
        for (float x : got.energy) finite = finite && isfinite(x);
        expect(finite, "nothing of a skipped view reaches the result");
    }

    // 4. refusals write nothing
    const Result two_tables = [&] {
        Result r{std::vector<float>((size_t)B * NQ, 7.0f), std::vector<float>((size_t)B, 7.0f), std::vector<float>((size_t)B, 7.0f), root0, 0};
        pndf_project_options10 o;
        memset(&o, 0, sizeof o);
        pndf_project_options6& o6 = o.base9.base8.base7.base6;
        o6.base5.base4.base3.base2.base.struct_size = sizeof o;
        o6.base5.base4.base3.base2.base.step_size = 1.0f;
        o6.base5.kp_target = target.data();
        o6.base5.rest = rest.data();
        o6.base5.n_keypoints = K;
        o6.base5.kp_joint = joint.data();
        o6.base5.nu = 0.1f;
        o6.root = r.root.data();
        o6.nu_trans = NU_TRANS;
        o6.kp_flags = PNDF_KP_IMAGE;
        o.base9.base8.views = fixed.data();
        o.base9.base8.n_views = V;
        o.pose_views = tiled.data();
        o.n_pose_views = V;
        r.rc = pndf_project_ex_cpu(h, q.data(), r.out.data(), r.d.data(), B, 1, (const pndf_project_options*)&o);
        return r;
    }();
    expect(two_tables.rc == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "one table or the other") && two_tables.out[0] == 7.0f &&
               same_bits(two_tables.root.data(), root0.data(), root0.size()),
           "both tables at once are refused and nothing is written");
    const Result flag = call(q, root0, 1, 1, tiled.data(), target, conf, 0.f, 0.f, 4u);
    expect(flag.rc == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "view_flags") && flag.out[0] == 7.0f && flag.energy[0] == 7.0f,
           "an unknown flag is refused and nothing is written");

    pndf_cpu_destroy(h);
    if (failures) return 1;
    printf("skeleton_cams_check: ok (15-joint hand, %d tracks of %d frames, 20 keypoints, %d moving cameras: reduction to the static call per pose and per "
           "frame, the path per frame against the path per pose, chained calls of both parities in both layouts, skipped views, refusals)\n", P, T, V);
    return 0;
}
