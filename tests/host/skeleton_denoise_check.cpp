// Stand-alone host program (own main, no HIP, no library): the host twin's denoising path -- pndf_project_ex_cpu with a
// pndf_project_options4 (include/posendf_amd.h) -- on a 15-joint hand with synthetic weights, three tracks of T = 5 frames, three steps,
// with a joint mask, confidences and free end frames.  Built with csrc/pndf_cpu.cpp in the same command; meant for a sanitizer build on
// the CPU,
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -pthread tests/host/skeleton_denoise_check.cpp
//         posendf_amd/csrc/pndf_cpu.cpp -o skeleton_denoise_check
// and checked without one by tests/test_skeleton_denoise_host.py.  Exit status 0 and one line that names what was checked.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/posendf_amd.h"

namespace {

const int32_t HAND[15] = {-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13};
constexpr int J = 15, NQ = 4 * J, P = 3, T = 5, B = P * T, STEPS = 3;

uint32_t rng_state = 24680u;
float uniform() {      // [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        printf("skeleton_denoise_check: FAILED %s\n", what);
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
        printf("skeleton_denoise_check: pndf_cpu_create failed: %s\n", pndf_cpu_last_error(nullptr));
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
        printf("skeleton_denoise_check: pndf_cpu_load_weights failed: %s\n", pndf_cpu_last_error(h));
        return 1;
    }
    // the noisy clip: three tracks of five frames, unit quaternions; the buffers are exactly as long as the call reads them, so a read
    // past an end frame's missing neighbour or past the confidences is one past an allocation
    std::vector<float> q((size_t)B * NQ), out((size_t)B * NQ, 7.0f), ref((size_t)B * NQ, 7.0f), d((size_t)B, 7.0f), dref((size_t)B, 7.0f);
    for (int i = 0; i < B * J; ++i) {
        float v[4], n = 0.f;
        for (float& x : v) {
            x = uniform() - 0.5f;
            n += x * x;
        }
        for (int c = 0; c < 4; ++c) q[(size_t)i * 4 + c] = v[c] / sqrtf(n);
    }
    // the observation: the clip itself, every third joint negated; the confidences in (0, 1], every fifth joint 0 with a NaN anchor
    std::vector<float> anchor = q, conf((size_t)B * J);
    for (int i = 0; i < B * J; ++i) {
        conf[(size_t)i] = 0.1f + 0.9f * uniform();
        if (i % 3 == 0)
            for (int c = 0; c < 4; ++c) anchor[(size_t)i * 4 + c] = -anchor[(size_t)i * 4 + c];
        if (i % 5 == 0) {
            conf[(size_t)i] = 0.f;
            for (int c = 0; c < 4; ++c) anchor[(size_t)i * 4 + c] = NAN;
        }
    }
    // the mask: every third joint of every frame of track 1 is held, end frames included
    std::vector<uint32_t> words((size_t)B, 0u);
    for (int k = 0; k < T; ++k) words[(size_t)(1 * T + k)] = 0x1249u << (k % 3);

    pndf_project_options4 o;
    o.base3.base2.base.struct_size = sizeof o;      // (pndf_default_project_options lives in the device library: the defaults by hand)
    o.base3.base2.base.step_size = 1.0f;
    o.base3.base2.base.tol = 0.0f;
    o.base3.base2.base.renorm = PNDF_RENORM_UNIT;
    o.base3.base2.observed = words.data();
    o.base3.base2.reserved = 0;
    o.base3.frames = T;
    o.base3.lambda = 0.5f;
    o.base3.fill = PNDF_TRACK_GIVEN;
    o.base3.reserved2 = 0;
    o.anchor = anchor.data();
    o.conf = conf.data();
    o.mu = 0.25f;
    o.flags = PNDF_TRACK_FREE_ENDS;
    const pndf_project_options* opt = (const pndf_project_options*)&o;

    // 1. three denoising steps: held joints keep their bits, every other joint moves (end frames included) and stays finite and unit
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "three denoising steps run");
    int moved = 0, free_joints = 0;
    for (int f = 0; f < B; ++f)
        for (int j = 0; j < J; ++j) {
            const size_t at = ((size_t)f * J + j) * 4;
            if ((words[(size_t)f] >> j) & 1u) {
                expect(same_bits(&out[at], &q[at], 4), "a held joint keeps its bits");
                continue;
            }
            ++free_joints;
            moved += !same_bits(&out[at], &q[at], 4);
            float n = 0.f;
            for (int c = 0; c < 4; ++c) {
                expect(isfinite(out[at + c]), "finite poses (a NaN anchor without confidence is not read)");
                n += out[at + c] * out[at + c];
            }
            expect(fabsf(n - 1.f) < 1e-5f, "unit quaternions");
        }
    expect(moved == free_joints, "every free joint moves, the end frames included");
    for (int f = 0; f < B; ++f) expect(isfinite(d[(size_t)f]), "finite distances");
    // 2. the data term holds the result nearer the observation than the same call without it
    o.mu = 0.f;
    expect(pndf_project_ex_cpu(h, q.data(), ref.data(), dref.data(), B, STEPS, opt) == 0, "mu = 0 runs (the NaN anchors are never read)");
    double tied = 0., loose = 0.;
    for (int i = 0; i < B * J; ++i) {
        if (conf[(size_t)i] <= 0.f) continue;
        double a = 0., b = 0.;
        for (int c = 0; c < 4; ++c) {
            a += (double)out[(size_t)i * 4 + c] * q[(size_t)i * 4 + c];
            b += (double)ref[(size_t)i * 4 + c] * q[(size_t)i * 4 + c];
        }
        tied += 1. - fabs(a);
        loose += 1. - fabs(b);
    }
    expect(tied < loose, "the data term keeps the clip nearer its observation");
    // 3. mu = 0 and no flag is the 48-byte call, bit for bit; so is anchor NULL
    o.flags = 0;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "mu = 0, held ends runs");
    pndf_project_options3 o3 = o.base3;
    o3.base2.base.struct_size = sizeof o3;
    expect(pndf_project_ex_cpu(h, q.data(), ref.data(), dref.data(), B, STEPS, (const pndf_project_options*)&o3) == 0, "the 48-byte call runs");
    expect(same_bits(out.data(), ref.data(), out.size()) && same_bits(d.data(), dref.data(), d.size()), "mu 0 without flags is the 48-byte call");
    o.anchor = nullptr;
    o.conf = nullptr;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "anchor NULL runs");
    expect(same_bits(out.data(), ref.data(), out.size()) && same_bits(d.data(), dref.data(), d.size()), "anchor NULL without flags is the 48-byte call");
    // 4. without tracks the call runs in place, the anchor elsewhere
    o.base3.frames = 0;
    o.base3.lambda = 0.f;
    o.anchor = anchor.data();
    o.conf = conf.data();
    o.mu = 0.25f;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "the data term without tracks runs");
    std::vector<float> inplace = q;
    expect(pndf_project_ex_cpu(h, inplace.data(), inplace.data(), dref.data(), B, STEPS, opt) == 0, "and in place");
    expect(same_bits(out.data(), inplace.data(), out.size()) && same_bits(d.data(), dref.data(), d.size()), "in place equals out of place");
    // 5. refusals write nothing
    std::fill(out.begin(), out.end(), 7.0f);
    o.flags = PNDF_TRACK_FREE_ENDS;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "FREE_ENDS"),
           "free ends without tracks are refused");
    o.flags = 0;
    o.mu = 1.5f;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "mu"), "mu > 1 is refused");
    o.mu = 0.25f;
    o.anchor = out.data();
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "anchor"),
           "an anchor in q_out is refused");
    for (float x : out) expect(x == 7.0f, "a refused call writes nothing");
    pndf_cpu_destroy(h);
    if (failures) {
        printf("skeleton_denoise_check: %d FAILURES\n", failures);
        return 1;
    }
    printf("skeleton_denoise_check: ok -- hand (15 joints), %d tracks of %d frames, %d steps, a joint mask, confidences and free end frames: the "
           "denoising step, the data term's pull, mu 0 and anchor NULL against the 48-byte call bit for bit, in place without tracks, 3 refusals\n",
           P, T, STEPS);
    return 0;
}
