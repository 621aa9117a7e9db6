// Stand-alone host program (own main, no HIP, no library): the host twin's several-camera path -- pndf_project_ex_cpu with a
// pndf_project_options8 (include/posendf_amd.h, the several-camera term of csrc/pndf_fk.h) -- on a 15-joint hand with synthetic weights,
// three tracks of T = 5 frames, three steps, K = 20 keypoints (the joints and a tip on every leaf) seen by V = 3 cameras around the scene,
// with confidences per view, a joint mask, the quaternion anchor, free end frames, the robustifier, a free root per pose and one row of
// scales per track.  Built with csrc/pndf_cpu.cpp in the same command; meant for a sanitizer build on the CPU,
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -pthread tests/host/skeleton_views_check.cpp
//         posendf_amd/csrc/pndf_cpu.cpp -o skeleton_views_check
// and checked without one by tests/test_skeleton_views_host.py.  Exit status 0 and one line that names what was checked.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/posendf_amd.h"

namespace {

const int32_t HAND[15] = {-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13};
constexpr int J = 15, NQ = 4 * J, P = 3, T = 5, B = P * T, STEPS = 3, K = J + 5, V = 3, S = J + K;

uint32_t rng_state = 24680u;
float uniform() {      // [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        printf("skeleton_views_check: FAILED %s\n", what);
        ++failures;
    }
}

bool same_bits(const float* a, const float* b, size_t n) { return memcmp(a, b, n * sizeof(float)) == 0; }

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
        printf("skeleton_views_check: pndf_cpu_create failed: %s\n", pndf_cpu_last_error(nullptr));
        return 1;
    }
    // the tensors in state-dict order: four per bone, then weight and bias of every trunk layer
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
        printf("skeleton_views_check: pndf_cpu_load_weights failed: %s\n", pndf_cpu_last_error(h));
        return 1;
    }
    // the start: three tracks of five frames, unit quaternions.  Every buffer is exactly as long as the call reads it -- the pixel targets
    // are [B][V][K][2], the confidences [B][V][K], the view table [V][16], the scales [P][S] -- so a read with the stride of one view, or
    // past the last view, is one past an allocation
    std::vector<float> q((size_t)B * NQ), out((size_t)B * NQ, 7.0f), ref((size_t)B * NQ, 7.0f), d((size_t)B, 7.0f), dref((size_t)B, 7.0f);
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
    // three cameras five units from the point (0, 0, 5) of the world frame, turned about its y axis by 0, 90 and 200 degrees
    std::vector<float> views((size_t)V * 16);
    const float angle[V] = {0.f, 1.5707963f, 3.4906585f};
    for (int v = 0; v < V; ++v) {
        float* r = &views[(size_t)v * 16];
        const float c = cosf(angle[v]), s = sinf(angle[v]);
        r[0] = 500.f + 20.f * v; r[1] = 480.f - 10.f * v; r[2] = 320.f; r[3] = 240.f + v;
        const float R[9] = {c, 0.f, s, 0.f, 1.f, 0.f, -s, 0.f, c};
        for (int i = 0; i < 9; ++i) r[4 + i] = R[i];
        r[13] = -s * 5.f; r[14] = 0.f; r[15] = 5.f - c * 5.f;      // t = (0, 0, 5) - R (0, 0, 5)
    }
    // pixel detections around the principal point and their confidences in (0, 1]; every seventh is missing: confidence 0, negative or NaN
    // and a NaN target
    std::vector<float> target((size_t)B * V * K * 2), kconf((size_t)B * V * K), energy((size_t)B, 7.0f), eref((size_t)B, 7.0f);
    for (int i = 0; i < B * V * K; ++i) {
        target[(size_t)i * 2] = 320.f + 150.f * (uniform() - 0.5f);
        target[(size_t)i * 2 + 1] = 240.f + 150.f * (uniform() - 0.5f);
        kconf[(size_t)i] = 0.1f + 0.9f * uniform();
        if (i % 7 == 0) {
            kconf[(size_t)i] = (i % 3 == 0) ? 0.f : (i % 3 == 1) ? -1.f : NAN;
            target[(size_t)i * 2] = target[(size_t)i * 2 + 1] = NAN;
        }
    }
    // the roots: raw quaternions near the identity, at the point the cameras look at; pose 4 has no view that sees it (every confidence 0)
    std::vector<float> root((size_t)B * 7), root0;
    for (int f = 0; f < B; ++f) {
        float* r = &root[(size_t)f * 7];
        r[0] = 1.5f;
        for (int c = 1; c < 4; ++c) r[c] = 0.3f * (uniform() - 0.5f);
        r[4] = 0.5f * (uniform() - 0.5f);
        r[5] = 0.5f * (uniform() - 0.5f);
        r[6] = 5.f + 0.5f * (uniform() - 0.5f);
    }
    for (int i = 0; i < V * K; ++i) {
        kconf[(size_t)4 * V * K + i] = 0.f;
        target[((size_t)4 * V * K + i) * 2] = target[((size_t)4 * V * K + i) * 2 + 1] = NAN;
    }
    root0 = root;
    std::vector<float> scale((size_t)P * S), scale0, rate((size_t)S, 1.0f);
    for (float& x : scale) x = 0.9f + 0.2f * uniform();
    for (int i = 0; i < S; i += 4) rate[(size_t)i] = 0.f;
    scale0 = scale;
    std::vector<float> anchor = q;
    std::vector<uint32_t> words((size_t)B, 0u);
    for (int k = 0; k < T; ++k) words[(size_t)(1 * T + k)] = 0x1249u << (k % 3);

    pndf_project_options8 o;
    memset(&o, 0, sizeof o);
    pndf_project_options7& o7 = o.base7;
    pndf_project_options6& o6 = o7.base6;
    pndf_project_options5& o5 = o6.base5;
    pndf_project_options& base = o5.base4.base3.base2.base;
    base.struct_size = sizeof o;      // (pndf_default_project_options lives in the device library: the defaults by hand)
    base.step_size = 1.0f;
    base.tol = 0.0f;
    base.renorm = PNDF_RENORM_UNIT;
    o5.base4.base3.base2.observed = words.data();
    o5.base4.base3.frames = T;
    o5.base4.base3.lambda = 0.5f;
    o5.base4.base3.fill = PNDF_TRACK_GIVEN;
    o5.base4.anchor = anchor.data();
    o5.base4.mu = 0.25f;
    o5.base4.flags = PNDF_TRACK_FREE_ENDS;
    o5.kp_target = target.data();
    o5.kp_conf = kconf.data();
    o5.kp_energy = energy.data();
    o5.rest = rest.data();
    o5.kp_joint = joint.data();
    o5.kp_offset = offset.data();
    o5.n_keypoints = K;
    o5.nu = 0.1f;
    o6.root = root.data();
    o6.fx = o6.fy = -1.f;      // with views the intrinsics of base6 are not read
    o6.rho = 0.25f;
    o6.nu_rot = 0.05f;
    o6.nu_trans = 0.1f;
    o6.kp_flags = PNDF_KP_IMAGE;
    o7.bone_scale = scale.data();
    o7.len_rate = rate.data();
    o7.nu_len = 0.05f;
    o7.kappa = 0.1f;
    o7.len_min = 0.5f;
    o7.len_max = 2.f;
    o.views = views.data();
    o.n_views = V;
    const pndf_project_options* opt = (const pndf_project_options*)&o;

    // 1. three steps: held joints keep their bits, the others stay finite and unit; energies finite; roots finite, their quaternions unit,
    //    their translations moved -- but for the pose no view sees, whose gradient is zero; scales finite, inside the clamp, moved where
    //    their rate is positive and the same bits where it is zero
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "three steps under three views run");
    for (int f = 0; f < B; ++f)
        for (int j = 0; j < J; ++j) {
            const size_t at = ((size_t)f * J + j) * 4;
            if ((words[(size_t)f] >> j) & 1u) {
                expect(same_bits(&out[at], &q[at], 4), "a held joint keeps its bits");
                continue;
            }
            float n = 0.f;
            for (int c = 0; c < 4; ++c) {
                expect(isfinite(out[at + c]), "finite poses (a NaN target without confidence is not read)");
                n += out[at + c] * out[at + c];
            }
            expect(fabsf(n - 1.f) < 1e-5f, "unit quaternions");
        }
    for (int f = 0; f < B; ++f) {
        expect(isfinite(d[(size_t)f]) && isfinite(energy[(size_t)f]) && (f == 4 ? energy[(size_t)f] == 0.f : energy[(size_t)f] > 0.f), "finite distances and energies");
        const float* r = &root[(size_t)f * 7];
        float n = 0.f;
        for (int c = 0; c < 7; ++c) expect(isfinite(r[c]), "finite roots");
        for (int c = 0; c < 4; ++c) n += r[c] * r[c];
        expect(fabsf(n - 1.f) < 1e-5f, "the root's quaternion is unit after a rotation step");
        expect(f == 4 ? same_bits(r + 4, &root0[(size_t)f * 7 + 4], 3) : !same_bits(r + 4, &root0[(size_t)f * 7 + 4], 3), "the root's translation moves where a view sees a keypoint");
    }
    for (int g = 0; g < P; ++g)
        for (int i = 0; i < S; ++i) {
            const size_t at = (size_t)g * S + i;
            expect(isfinite(scale[at]) && scale[at] >= 0.5f && scale[at] <= 2.f, "finite scales inside the clamp");
            expect(i % 4 == 0 ? same_bits(&scale[at], &scale0[at], 1) : !same_bits(&scale[at], &scale0[at], 1), "a scale moves exactly where its rate is positive");
        }
    // 2. the term lowers the energy: ten steps without tracks and without scales end below where they started
    std::vector<float> e0((size_t)B), e1((size_t)B), mid((size_t)B * NQ), r_mid;
    o5.base4.base3.base2.observed = nullptr;
    o5.base4.base3.frames = 0;
    o5.base4.base3.lambda = 0.f;
    o5.base4.anchor = nullptr;
    o5.base4.mu = 0.f;
    o5.base4.flags = 0;
    o6.rho = 0.f;
    o7.bone_scale = nullptr;
    o7.nu_len = 0.f;
    root = root0;
    o5.kp_energy = e0.data();
    expect(pndf_project_ex_cpu(h, q.data(), mid.data(), d.data(), B, 1, opt) == 0, "one step without tracks runs");
    root = root0;
    o5.kp_energy = e1.data();
    expect(pndf_project_ex_cpu(h, q.data(), mid.data(), d.data(), B, 10, opt) == 0, "ten steps without tracks run");
    r_mid = root;
    double before = 0., after = 0.;
    for (int f = 0; f < B; ++f) {
        before += e0[(size_t)f];
        after += e1[(size_t)f];
    }
    expect(after < before, "the summed energy falls");
    // 3. in place equals out of place, roots included
    std::vector<float> inplace = q;
    root = root0;
    o5.kp_energy = eref.data();
    expect(pndf_project_ex_cpu(h, inplace.data(), inplace.data(), dref.data(), B, 10, opt) == 0, "and in place");
    expect(same_bits(mid.data(), inplace.data(), mid.size()) && same_bits(d.data(), dref.data(), d.size()) && same_bits(e1.data(), eref.data(), e1.size()) &&
               same_bits(root.data(), r_mid.data(), root.size()),
           "in place equals out of place");
    // 4. one view with R = I, t = 0: the 208-byte call with that camera (compared by value: the identity products may turn -0 into +0);
    //    views NULL and n_views 0: the 208-byte call, bit for bit.  Targets [B][K][2]: the first view's stride is the only one
    std::vector<float> target1((size_t)B * K * 2), conf1((size_t)B * K);
    for (int i = 0; i < B * K; ++i) {
        target1[(size_t)i * 2] = 320.f + 150.f * (uniform() - 0.5f);
        target1[(size_t)i * 2 + 1] = 240.f + 150.f * (uniform() - 0.5f);
        conf1[(size_t)i] = i % 5 ? 0.1f + 0.9f * uniform() : 0.f;
    }
    const float ident[16] = {500.f, 480.f, 320.f, 240.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    o5.base4.base3.base2.observed = words.data();
    o5.base4.base3.frames = T;
    o5.base4.base3.lambda = 0.5f;
    o5.base4.anchor = anchor.data();
    o5.base4.mu = 0.25f;
    o5.base4.flags = PNDF_TRACK_FREE_ENDS;
    o5.kp_target = target1.data();
    o5.kp_conf = conf1.data();
    o6.rho = 0.25f;
    o6.fx = 500.f; o6.fy = 480.f; o6.cx = 320.f; o6.cy = 240.f;
    o7.bone_scale = scale.data();
    o7.nu_len = 0.05f;
    pndf_project_options7 small = o7;
    small.base6.base5.base4.base3.base2.base.struct_size = sizeof small;
    small.base6.base5.kp_energy = eref.data();
    std::vector<float> root_ref, scale_ref;
    root = root0;
    scale = scale0;
    expect(pndf_project_ex_cpu(h, q.data(), ref.data(), dref.data(), B, STEPS, (const pndf_project_options*)&small) == 0, "the 208-byte call runs");
    root_ref = root;
    scale_ref = scale;
    auto same_values = [](const std::vector<float>& a, const std::vector<float>& b) {
        for (size_t i = 0; i < a.size(); ++i)
            if (!(a[i] == b[i]) && !(a[i] != a[i] && b[i] != b[i])) return false;
        return true;
    };
    o5.kp_energy = energy.data();
    for (int pass = 0; pass < 2; ++pass) {
        o.views = pass ? nullptr : ident;
        o.n_views = pass ? 0 : 1;
        root = root0;
        scale = scale0;
        expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, pass ? "no views runs" : "one identity view runs");
        if (pass)
            expect(same_bits(out.data(), ref.data(), out.size()) && same_bits(d.data(), dref.data(), d.size()) && same_bits(energy.data(), eref.data(), energy.size()) &&
                       same_bits(root.data(), root_ref.data(), root.size()) && same_bits(scale.data(), scale_ref.data(), scale.size()),
                   "no views is the 208-byte call");
        else
            expect(same_values(out, ref) && same_values(d, dref) && same_values(energy, eref) && same_values(root, root_ref) && same_values(scale, scale_ref),
                   "one identity view is the 208-byte call");
    }
    // 5. nu = 0: the 72-byte call; targets, confidences, root and scales full of NaN are neither read nor written
    pndf_project_options4 o4 = o5.base4;
    o4.base3.base2.base.struct_size = sizeof o4;
    expect(pndf_project_ex_cpu(h, q.data(), ref.data(), dref.data(), B, STEPS, (const pndf_project_options*)&o4) == 0, "the 72-byte call runs");
    std::vector<float> nan_root((size_t)B * 7, NAN), nan_copy = nan_root, nan_scale((size_t)P * S, NAN), nan_target((size_t)B * V * K * 2, NAN), nan_conf((size_t)B * V * K, NAN);
    o6.root = nan_root.data();
    o7.bone_scale = nan_scale.data();
    o5.kp_target = nan_target.data();
    o5.kp_conf = nan_conf.data();
    o5.nu = 0.f;
    o.views = views.data();
    o.n_views = V;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "nu = 0 runs");
    expect(same_bits(out.data(), ref.data(), out.size()) && same_bits(d.data(), dref.data(), d.size()), "nu 0 is the 72-byte call");
    expect(same_bits(nan_root.data(), nan_copy.data(), nan_root.size()), "a root nobody reads is not written");
    for (float x : nan_scale) expect(x != x, "scales nobody reads are not written");
    for (float x : energy) expect(x == 0.f, "nu 0 zeroes the energies");
    // 6. refusals write nothing
    o5.nu = 0.1f;
    o5.kp_target = target.data();
    o5.kp_conf = kconf.data();
    o6.root = root.data();
    o7.bone_scale = scale.data();
    root = root0;
    scale = scale0;
    std::fill(out.begin(), out.end(), 7.0f);
    std::fill(energy.begin(), energy.end(), 7.0f);
    auto refused = [&](const char* field, const char* what) {
        expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), field), what);
    };
    o.reserved4 = 1;
    refused("reserved4", "a reserved word that is not 0 is refused");
    o.reserved4 = 0;
    o.n_views = 9;
    refused("n_views must lie in", "nine views are refused");
    o.n_views = 0;
    refused("n_views must be positive", "views without a count are refused");
    o.n_views = V;
    o.views = nullptr;
    refused("views must not be NULL", "a count without views is refused");
    o.views = views.data();
    o6.kp_flags = 0;
    o6.rho = 0.f;
    refused("kp_flags", "views without PNDF_KP_IMAGE are refused");
    o6.kp_flags = PNDF_KP_IMAGE;
    std::vector<float> bad_views = views;
    bad_views[16] = 0.f;
    o.views = bad_views.data();
    refused("fx", "fx = 0 in a view is refused");
    bad_views = views;
    bad_views[2 * 16 + 9] = NAN;
    refused("views has an entry that is not finite", "a NaN in a view's rotation is refused");
    o.views = views.data();
    std::vector<float> arena((size_t)B * V * K * 2 - 1 + (size_t)B * NQ, 7.0f);      // targets at its start, q_out over their last float
    o5.kp_target = arena.data();
    expect(pndf_project_ex_cpu(h, q.data(), arena.data() + ((size_t)B * V * K * 2 - 1), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG &&
               strstr(pndf_cpu_last_error(h), "kp_target"),
           "targets [B,V,K,2] whose last float lies in q_out are refused");
    for (float x : arena) expect(x == 7.0f, "a refused call writes nothing");
    o5.kp_target = target.data();
    for (float x : out) expect(x == 7.0f, "a refused call writes nothing");
    for (float x : energy) expect(x == 7.0f, "a refused call writes no energy");
    expect(same_bits(root.data(), root0.data(), root.size()) && same_bits(scale.data(), scale0.data(), scale.size()), "a refused call writes no root and no scale");
    pndf_cpu_destroy(h);
    if (failures) {
        printf("skeleton_views_check: %d FAILURES\n", failures);
        return 1;
    }
    printf("skeleton_views_check: ok -- hand (15 joints), %d keypoints in %d views, %d tracks of %d frames, %d steps, a joint mask, the anchor, confidences per "
           "view with NaN targets, free end frames, the robustifier, a free root per pose, a pose no view sees and one row of %d scales per track: the step, the "
           "energy's fall, in place without tracks, one identity view and no views against the 208-byte call, the 72-byte call bit for bit with NaN arrays "
           "that are not read, 8 refusals\n", K, V, P, T, STEPS, S);
    return 0;
}
