// Host twins of the three compute entry points (`pndf_*_cpu`): the same contract as pndf_forward /
// pndf_forward_grad / pndf_project (include/posendf_amd.h) on HOST pointers, for a caller whose `train.device` is "cpu"
// (reference model/posendf.py:35,64 moves the pose to whatever device the config names).  Written from scratch in plain
// C++ for the host cores -- NOT the oracle (oracle/ is test infrastructure and is imported by nothing here) and NOT a
// fallback: the device entry points never route here, a missing GPU still fails loudly there.  The first-order twins take the joint
// count and the parent table from the handle's config (any joint tree of include/posendf_amd_skeleton.h, pndf_net_plan.h); on the
// SMPL table they compute what they did with the table fixed.  pndf_complete_cpu, pndf_interpolate_cpu and the second order stay 21-joint;
// pndf_project_ex_cpu completes, interpolates, denoises and fits 3D or 2D keypoints for any joint tree (pndf_project_options2 /
// pndf_project_options3 / pndf_project_options4 / pndf_project_options5 / pndf_project_options6), with the bone lengths as unknowns too
// (pndf_project_options7), the pixels seen by several calibrated cameras (pndf_project_options8), the root's trajectory over the
// frames of a track (pndf_project_options9) and cameras that move from pose to pose or frame to frame (pndf_project_options10).
//
// Layout: poses are processed in blocks of PB = 32; inside a block every activation tensor is [feature][pose] so that the
// inner loop of a layer runs over the 32 poses of the block (contiguous floats: one or two AVX-512 / four AVX2 registers)
// with the weight as a broadcast scalar, four output rows at a time.  The backward pass runs the same loop on transposed
// copies of the weights made once at load time.  Blocks are dealt to std::threads (PNDF_CPU_THREADS, default: the
// hardware concurrency, at most one thread per block).  Arithmetic is fp32 throughout; the activation conventions are
// PyTorch's (nn.LeakyReLU slope 0.01 with derivative `x > 0 ? 1 : slope`, nn.ReLU on the output of the relu family,
// nn.Softplus(beta, threshold 20) and softplus_backward's e / (e + 1)); F.normalize(dim=1) with eps 1e-12; the update
// q - d * grad keeps the reference's two roundings (sample_poses.py:74).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/posendf_amd.h"
#include "../../include/posendf_amd_completion.h"
#include "../../include/posendf_amd_second_order.h"
#include "pndf_error.h"
#include "pndf_fk.h"
#include "pndf_interp.h"
#include "pndf_layout.h"
#include "pndf_online.h"
#include "../../include/posendf_amd_skeleton_data.h"
#include "pndf_project_opts.h"
#include "pndf_net_plan.h"

using namespace pndf;

namespace {

constexpr int PB = 32;
constexpr int MAXJ = PNDF_SKEL_MAX_JOINTS;      // the first-order twins take any joint tree (pndf_net_plan.h); the others stay 21-joint

struct Layer {
    int in = 0, out = 0;
    std::vector<float> w, wt, b;      // w [out][in], wt [in][out], b [out]
};

}  // namespace

struct pndf_cpu_engine {
    LayerNet net;           // the skeleton, the widths, the activations and the size of every tensor (pndf_net_plan.h)
    bool have_weights = false;
    bool smpl = true;       // 21 joints along get_parent_mapping('smpl'): what completion, interpolation and the second order need
    Layer enc[MAXJ][2];
    Layer lin[MAXLIN];      // any DFNet depth the reference can build (net_modules.py:14-28: `dims` is a free list): 2 .. 8 linear layers
    std::string err;
    int nq() const { return 4 * net.nj; }      // quaternion components of a pose
};

namespace {

// y[o][p] = b[o] + sum_i w[o][i] x[i][p]   (four rows of y at a time; the compiler vectorises the p loops)
__attribute__((target_clones("avx512f", "arch=haswell", "default")))
void dense(const float* w, const float* b, int out, int in, const float* x, float* y) {
    int o = 0;
    for (; o + 4 <= out; o += 4) {
        float a0[PB], a1[PB], a2[PB], a3[PB];
        for (int p = 0; p < PB; ++p) {
            a0[p] = b ? b[o] : 0.f; a1[p] = b ? b[o + 1] : 0.f; a2[p] = b ? b[o + 2] : 0.f; a3[p] = b ? b[o + 3] : 0.f;
        }
        const float *w0 = w + (size_t)o * in, *w1 = w0 + in, *w2 = w1 + in, *w3 = w2 + in;
        for (int i = 0; i < in; ++i) {
            const float* xi = x + (size_t)i * PB;
            const float c0 = w0[i], c1 = w1[i], c2 = w2[i], c3 = w3[i];
            for (int p = 0; p < PB; ++p) {
                a0[p] += c0 * xi[p]; a1[p] += c1 * xi[p]; a2[p] += c2 * xi[p]; a3[p] += c3 * xi[p];
            }
        }
        memcpy(y + (size_t)o * PB, a0, sizeof(a0)); memcpy(y + (size_t)(o + 1) * PB, a1, sizeof(a1));
        memcpy(y + (size_t)(o + 2) * PB, a2, sizeof(a2)); memcpy(y + (size_t)(o + 3) * PB, a3, sizeof(a3));
    }
    for (; o < out; ++o) {
        float a0[PB];
        for (int p = 0; p < PB; ++p) a0[p] = b ? b[o] : 0.f;
        const float* w0 = w + (size_t)o * in;
        for (int i = 0; i < in; ++i) {
            const float* xi = x + (size_t)i * PB;
            const float c0 = w0[i];
            for (int p = 0; p < PB; ++p) a0[p] += c0 * xi[p];
        }
        memcpy(y + (size_t)o * PB, a0, sizeof(a0));
    }
}

struct Act {
    int kind;      // pndf_act
    float beta;
};

// in place: z -> act(z); der <- act'(z)   (n values)
void activate(const Act& a, float* z, float* der, int n, bool output_layer) {
    if (a.kind == PNDF_ACT_SOFTPLUS) {
        for (int i = 0; i < n; ++i) {
            const float bz = z[i] * a.beta;
            if (bz > 20.0f) {
                der[i] = 1.0f;
            } else {
                const float e = expf(bz);
                der[i] = e / (e + 1.0f);
                z[i] = log1pf(e) / a.beta;
            }
        }
        return;
    }
    const float slope = (a.kind == PNDF_ACT_LRELU && !output_layer) ? 0.01f : 0.0f;      // net_modules.py:30-37
    for (int i = 0; i < n; ++i) {
        const bool pos = z[i] > 0.0f;
        der[i] = pos ? 1.0f : slope;
        // relu(NaN) = NaN, lrelu(NaN) = NaN as in PyTorch
        z[i] = (z[i] != z[i]) ? z[i] : (pos ? z[i] : z[i] * slope);
    }
}

struct Scratch {      // per thread
    std::vector<float> n, x[MAXLIN + 1], dx[MAXLIN + 1], g, g2, eh[MAXJ], ehd[MAXJ], ef[MAXJ], efd[MAXJ], ein[MAXJ], gf, gh, gin;
    float inv[4][PB], nrm[4][PB];
};

void forward_grad_block(const pndf_cpu_engine& E, const float* q /*[nb][4 nj]*/, int nb, const float* gout, float* d, float* dq,
                        bool want_grad, Scratch& S) {
    const int NJ = E.net.nj, NQ = E.nq(), NFEAT = FEAT * NJ;      // the skeleton of the handle (shadowing pndf_layout.h's SMPL constants)
    const int* PARENT = E.net.parent;
    auto enc_in = [PARENT](int j) { return PARENT[j] < 0 ? 4 : 10; };
    const Act act{E.net.act, E.net.beta};
    const Act eact{E.net.enc_act, E.net.enc_beta};      // model.StrEnc.act / beta, read on their own (net_modules.py:128)
    // ---- normalise over joints per component (posendf.py:71), poses of the block as the inner index
    S.n.assign((size_t)NQ * PB, 0.f);
    for (int c = 0; c < 4; ++c)
        for (int p = 0; p < PB; ++p) {
            float ss = 0.f;
            if (p < nb)
                for (int j = 0; j < NJ; ++j) ss += q[(size_t)p * NQ + 4 * j + c] * q[(size_t)p * NQ + 4 * j + c];
            const float norm = sqrtf(ss);
            S.nrm[c][p] = norm;
            S.inv[c][p] = 1.0f / std::max(norm, 1e-12f);
        }
    for (int j = 0; j < NJ; ++j)
        for (int c = 0; c < 4; ++c)
            for (int p = 0; p < nb; ++p) S.n[(size_t)(4 * j + c) * PB + p] = q[(size_t)p * NQ + 4 * j + c] * S.inv[c][p];
    // ---- structure encoder (net_modules.py:140-170) or the normalised pose itself
    const int d0 = E.net.dims[0];
    S.x[0].assign((size_t)d0 * PB, 0.f);
    if (E.net.encoder) {
        for (int j = 0; j < NJ; ++j) {
            const int in = enc_in(j);
            S.ein[j].assign((size_t)in * PB, 0.f);
            memcpy(S.ein[j].data(), &S.n[(size_t)4 * j * PB], sizeof(float) * 4 * PB);
            if (PARENT[j] >= 0) memcpy(S.ein[j].data() + 4 * PB, S.ef[PARENT[j]].data(), sizeof(float) * FEAT * PB);
            S.eh[j].resize((size_t)HID * PB); S.ehd[j].resize((size_t)HID * PB);
            S.ef[j].resize((size_t)FEAT * PB); S.efd[j].resize((size_t)FEAT * PB);
            dense(E.enc[j][0].w.data(), E.enc[j][0].b.data(), HID, in, S.ein[j].data(), S.eh[j].data());
            activate(eact, S.eh[j].data(), S.ehd[j].data(), HID * PB, false);
            dense(E.enc[j][1].w.data(), E.enc[j][1].b.data(), FEAT, HID, S.eh[j].data(), S.ef[j].data());
            activate(eact, S.ef[j].data(), S.efd[j].data(), FEAT * PB, false);
            memcpy(&S.x[0][(size_t)FEAT * j * PB], S.ef[j].data(), sizeof(float) * FEAT * PB);      // cat(f_0 .. f_20), :169
        }
    } else {
        memcpy(S.x[0].data(), S.n.data(), sizeof(float) * NQ * PB);
    }
    // ---- DFNet (net_modules.py:46-72)
    const int NL = E.net.L;
    for (int l = 0; l < NL; ++l) {
        const Layer& L = E.lin[l];
        S.x[l + 1].resize((size_t)L.out * PB);
        S.dx[l + 1].resize((size_t)L.out * PB);
        dense(L.w.data(), L.b.data(), L.out, L.in, S.x[l].data(), S.x[l + 1].data());
        activate(act, S.x[l + 1].data(), S.dx[l + 1].data(), L.out * PB, l == NL - 1);
    }
    for (int p = 0; p < nb; ++p) d[p] = S.x[NL][p];
    if (!want_grad) return;
    // ---- d (sum_b grad_out_b d_b) / d q: reverse pass
    S.g.assign((size_t)PB, 0.f);
    for (int p = 0; p < nb; ++p) S.g[p] = (gout ? gout[p] : 1.0f) * S.dx[NL][p];
    for (int l = NL - 1; l >= 0; --l) {
        const Layer& L = E.lin[l];
        S.g2.resize((size_t)L.in * PB);
        dense(L.wt.data(), nullptr, L.in, L.out, S.g.data(), S.g2.data());
        if (l > 0)
            for (size_t i = 0; i < (size_t)L.in * PB; ++i) S.g2[i] *= S.dx[l][i];
        S.g.swap(S.g2);
    }
    // S.g = d / d x0  [d0][PB]
    std::vector<float>& gn = S.g2;
    gn.assign((size_t)NQ * PB, 0.f);
    if (E.net.encoder) {
        // children before parents: joints in decreasing index order (every parent has a smaller index)
        std::vector<float>& gfeat = S.gf;
        gfeat.assign(S.g.begin(), S.g.begin() + (size_t)NFEAT * PB);      // accumulates the children's contributions
        for (int j = NJ - 1; j >= 0; --j) {
            const int in = enc_in(j);
            float* gfj = &gfeat[(size_t)FEAT * j * PB];
            for (int i = 0; i < FEAT * PB; ++i) gfj[i] *= S.efd[j][i];
            S.gh.resize((size_t)HID * PB);
            dense(E.enc[j][1].wt.data(), nullptr, HID, FEAT, gfj, S.gh.data());
            for (int i = 0; i < HID * PB; ++i) S.gh[i] *= S.ehd[j][i];
            S.gin.resize((size_t)in * PB);
            dense(E.enc[j][0].wt.data(), nullptr, in, HID, S.gh.data(), S.gin.data());
            memcpy(&gn[(size_t)4 * j * PB], S.gin.data(), sizeof(float) * 4 * PB);
            if (PARENT[j] >= 0) {
                float* gp = &gfeat[(size_t)FEAT * PARENT[j] * PB];
                for (int i = 0; i < FEAT * PB; ++i) gp[i] += S.gin[(size_t)4 * PB + i];
            }
        }
    } else {
        memcpy(gn.data(), S.g.data(), sizeof(float) * NQ * PB);
    }
    // ---- F.normalize backward: n = q / max(||q_c||, eps) per component column
    for (int c = 0; c < 4; ++c)
        for (int p = 0; p < nb; ++p) {
            float dot = 0.f;
            for (int j = 0; j < NJ; ++j) dot += gn[(size_t)(4 * j + c) * PB + p] * q[(size_t)p * NQ + 4 * j + c];
            const float norm = S.nrm[c][p], den = std::max(norm, 1e-12f);
            const float kk = (norm > 1e-12f) ? dot / (den * den * norm) : 0.f;      // the clamped branch has no norm term
            for (int j = 0; j < NJ; ++j)
                dq[(size_t)p * NQ + 4 * j + c] = gn[(size_t)(4 * j + c) * PB + p] / den - q[(size_t)p * NQ + 4 * j + c] * kk;
        }
}

int threads_for(int64_t blocks) {
    int n = (int)std::thread::hardware_concurrency();
    if (const char* e = getenv("PNDF_CPU_THREADS")) n = atoi(e);
    if (n < 1) n = 1;
    return (int)std::min<int64_t>(n, blocks);
}

// (throws std::runtime_error when a worker or a thread start failed: the entry points turn it into PNDF_ERR_HOST)
template <class F>
void parallel_blocks(int64_t B, F&& body) {
    const int64_t blocks = (B + PB - 1) / PB;
    const int nt = threads_for(blocks);
    std::atomic<bool> failed{false};
    auto worker = [&](int t) {
        try {
            Scratch S;
            for (int64_t blk = t; blk < blocks && !failed.load(std::memory_order_relaxed); blk += nt)
                body(blk * PB, (int)std::min<int64_t>(PB, B - blk * PB), S);
        } catch (...) {      // (an allocation of the scratch: nothing else in a block throws)
            failed.store(true);
        }
    };
    if (nt == 1) {
        worker(0);
    } else {
        std::vector<std::thread> pool;
        try {
            for (int t = 1; t < nt; ++t) pool.emplace_back(worker, t);
        } catch (...) {
            failed.store(true);      // the blocks of the threads that did not start stay undone: the call fails as a whole
        }
        if (!failed.load()) worker(0);
        for (auto& th : pool) th.join();
    }
    if (failed.load()) throw std::runtime_error("a worker thread could not be started or ran out of memory");
}

int check(pndf_cpu_engine* h, const void* q, int64_t B) {
    if (!h) return PNDF_ERR_BAD_ARG;
    if (!h->have_weights) return pndf_fail(h, PNDF_ERR_NO_WEIGHTS, "pndf_cpu_load_weights has not been called");
    if (B < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative batch");
    if (B > 0 && !q) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pose pointer");
    return PNDF_OK;
}

// No C++ exception may cross the C ABI: a failed thread start or allocation becomes a status code with its text.
template <class F>
int guarded(pndf_cpu_engine* h, F&& body) {
    try {
        body();
        return PNDF_OK;
    } catch (const std::exception& e) {
        return pndf_fail(h, PNDF_ERR_HOST, std::string("host resource failure: ") + e.what());
    } catch (...) {
        return pndf_fail(h, PNDF_ERR_HOST, "host resource failure");
    }
}

}  // namespace

extern "C" int pndf_cpu_create(pndf_cpu_handle* out, const pndf_config* cfg) {
    if (!out || !cfg) return pndf_fail<pndf_cpu_engine>(nullptr, PNDF_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    // any joint tree (include/posendf_amd_skeleton.h): 1 .. 32 joints, every parent before its child, dims[0] = 6 J or 4 J; the
    // same DFNets the device units accept
    if (const char* why = pndf_skeleton_refusal(cfg)) return pndf_fail<pndf_cpu_engine>(nullptr, PNDF_ERR_UNSUPPORTED, why);
    if (const char* why = pndf_dfnet_refusal(cfg)) return pndf_fail<pndf_cpu_engine>(nullptr, PNDF_ERR_UNSUPPORTED, why);
    if (cfg->act == PNDF_ACT_SOFTPLUS && !(cfg->beta > 0.f)) return pndf_fail<pndf_cpu_engine>(nullptr, PNDF_ERR_BAD_ARG, "Softplus beta must be positive");
    if (cfg->enc_act == PNDF_ACT_SOFTPLUS && !(cfg->enc_beta > 0.f) && !(cfg->beta > 0.f)) return pndf_fail<pndf_cpu_engine>(nullptr, PNDF_ERR_BAD_ARG, "Softplus beta of the encoder must be positive");
    return guarded(nullptr, [&] {
        pndf_cpu_engine* h = new pndf_cpu_engine();
        layer_net_init(h->net, cfg, -1);      // (no device)
        h->smpl = pndf_skeleton_is_smpl(cfg);
        *out = h;
    });
}

extern "C" int pndf_cpu_destroy(pndf_cpu_handle h) {
    delete h;
    return PNDF_OK;
}

extern "C" const char* pndf_cpu_last_error(pndf_cpu_handle h) { return pndf_last_error_of(h); }

extern "C" int pndf_cpu_load_weights(pndf_cpu_handle h, const float* const* tensors, const int64_t* numel, int n_tensors) {
    if (!h) return PNDF_ERR_BAD_ARG;
    const PndfTableFault f = pndf_table_fault(h->net, tensors, numel, n_tensors);
    if (f.kind == PndfTableFault::NULL_TABLE) return PNDF_ERR_BAD_ARG;
    if (f.kind == PndfTableFault::COUNT) return pndf_fail(h, PNDF_ERR_BAD_SHAPE, f.text());
    h->have_weights = false;      // a table of the right length that does not fit leaves the handle without weights, as a failed copy does
    if (f) return pndf_fail(h, PNDF_ERR_BAD_SHAPE, f.text());
    const int grc = guarded(h, [&] {
        int t = 0;
        auto take = [&](Layer& L, int out, int in) {
            L.in = in; L.out = out;
            L.w.assign(tensors[t], tensors[t] + (size_t)out * in);
            L.b.assign(tensors[t + 1], tensors[t + 1] + out);
            L.wt.resize((size_t)in * out);
            for (int o = 0; o < out; ++o)
                for (int i = 0; i < in; ++i) L.wt[(size_t)i * out + o] = L.w[(size_t)o * in + i];
            t += 2;
        };
        for (int j = 0; h->net.encoder && j < h->net.nj; ++j) {
            take(h->enc[j][0], HID, h->net.parent[j] < 0 ? 4 : 10);
            take(h->enc[j][1], FEAT, HID);
        }
        for (int l = 0; l < h->net.L; ++l) take(h->lin[l], h->net.dims[l + 1], h->net.dims[l]);
    });
    if (grc != PNDF_OK) return grc;
    h->have_weights = true;
    return PNDF_OK;
}

extern "C" int pndf_forward_cpu(pndf_cpu_handle h, const float* q, float* d, int64_t B) {
    if (int rc = check(h, q, B)) return rc;
    if (B > 0 && !d) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null output pointer");
    return guarded(h, [&] {
        parallel_blocks(B, [&](int64_t p0, int nb, Scratch& S) { forward_grad_block(*h, q + p0 * h->nq(), nb, nullptr, d + p0, nullptr, false, S); });
    });
}

extern "C" int pndf_forward_grad_cpu(pndf_cpu_handle h, const float* q, const float* grad_out, float* d, float* dq, int64_t B) {
    if (int rc = check(h, q, B)) return rc;
    if (B > 0 && !dq) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null output pointer");
    return guarded(h, [&] {
        parallel_blocks(B, [&](int64_t p0, int nb, Scratch& S) {
            float dd[PB];
            forward_grad_block(*h, q + p0 * h->nq(), nb, grad_out ? grad_out + p0 : nullptr, dd, dq + p0 * h->nq(), true, S);
            if (d) memcpy(d + p0, dd, sizeof(float) * nb);
        });
    });
}

extern "C" int pndf_project_cpu(pndf_cpu_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps) {
    if (int rc = check(h, q_in, B)) return rc;
    if (steps < 0 || (B > 0 && !q_out)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative step count or null output pointer");
    const int NQ = h->nq();
    return guarded(h, [&] {
    parallel_blocks(B, [&](int64_t p0, int nb, Scratch& S) {
        float qb[PB * 4 * MAXJ], dqb[PB * 4 * MAXJ], dd[PB];
        memcpy(qb, q_in + p0 * NQ, sizeof(float) * nb * NQ);
        for (int p = 0; p < nb; ++p) dd[p] = 0.f;
        for (int s = 0; s < steps; ++s) {
            forward_grad_block(*h, qb, nb, nullptr, dd, dqb, true, S);
            for (int p = 0; p < nb; ++p)
                for (int i = 0; i < NQ; ++i) {
                    volatile float prod = dd[p] * dqb[p * NQ + i];      // two roundings, as the reference evaluates q - d * grad
                    qb[p * NQ + i] = qb[p * NQ + i] - prod;
                }
        }
        memcpy(q_out + p0 * NQ, qb, sizeof(float) * nb * NQ);
        if (d_last) memcpy(d_last + p0, dd, sizeof(float) * nb);
    });
    });
}

// pndf_interpolate_cpu, the second order and pndf_complete_cpu themselves stay 21-joint; another skeleton completes
// poses through pndf_project_ex_cpu with a pndf_project_options2 and interpolates through it with a pndf_project_options3
static const char* const SMPL_ONLY = "this entry point runs the 21-joint table of get_parent_mapping('smpl') only; a handle of another skeleton "
                                     "has pndf_forward_cpu, pndf_forward_grad_cpu, pndf_project_cpu and pndf_project_ex_cpu (which holds "
                                     "observed joints when it is given a pndf_project_options2 and interpolates tracks when it is given a "
                                     "pndf_project_options3)";

// One step of pndf_project_ex on the host: pndf_step.h's pndf_step_quat -- the statement the device kernels run -- for every joint of
// a pose that does not rest.  `held`: bit j = joint j is observed and stays as it is (pndf_complete_cpu, and pndf_project_ex_cpu with the
// mask of a pndf_project_options2; without one it holds none).  `anchor` / `conf`: the pose's rows of the observation of a
// pndf_project_options4 (null: none): then the step is pndf_interp.h's pndf_denoise_quat without neighbours, the data term alone.
// The host tables of a pndf_project_options5 with their defaults filled in (pndf_fill_keypoint_tables), as the kernel's arguments hold them
struct KeypointTables {
    float rest[3 * MAXJ];
    int32_t kpj[PNDF_FK_MAX_KEYPOINTS];
    float kpo[3 * PNDF_FK_MAX_KEYPOINTS];
};

// The root buffers of a step with the trajectory of a pndf_project_options9: every frame reads its own and its neighbours' rows in `src`
// and writes its row of `dst` (the same array only without tracks, where no frame reads another's row); frames: T, or 0
struct RootTrack {
    const PndfRootSmooth* rs;
    const float* src;
    float* dst;
    int32_t frames;
};

// The root's own step of pose number `pose`: pndf_fk_root_step in place, or with a pndf_project_options9 (`tr`) pndf_fk_root_smooth_step
// from tr->src to tr->dst.  root: the row at the step's input, as the term read it.
static void root_step_cpu(const PndfCameraTerm& cam, float* rt, const float* root, const float* groot, float dist, float tol, int64_t pose,
                          const RootTrack* tr) {
    float stepped[7];
    if (!tr) {
        if (!cam.moves()) return;
        pndf_fk_root_step(root, groot, cam.nu_rot, cam.nu_trans, dist, tol, stepped);
        memcpy(rt, stepped, sizeof(stepped));
        return;
    }
    const int k = tr->frames ? (int)(pose % tr->frames) : 0;
    const int nbr = tr->frames ? ((k > 0 ? 1 : 0) | (k < tr->frames - 1 ? 2 : 0)) : 0;
    const float* row = tr->src + pose * 7;
    const PndfRootSmooth& rs = *tr->rs;
    pndf_fk_root_smooth_step(root, groot, cam.nu_rot, cam.nu_trans, dist, tol, (nbr & 1) ? row - 7 : nullptr, (nbr & 2) ? row + 7 : nullptr, nbr,
                             rs.lambda_rot, rs.lambda_trans, rs.anchor ? rs.anchor + pose * 7 : nullptr, rs.mu_rot, rs.mu_trans, stepped);
    memcpy(tr->dst + pose * 7, stepped, sizeof(stepped));
}

// The keypoint term of pose number `pose` at the iterate q: pndf_fk.h's pndf_fk_energy_grad -- the statement the device kernel runs -- on
// a local array of rows (ld = 1).  gk [nj][4] = d E / d Q; returns E.  With the camera or the root of a pndf_project_options6 (`cam`) the
// term is pndf_fk_camera_energy_grad, and the pose's root row takes its own step here (pndf_fk_root_step; `dist` and `tol` say whether
// the pose rests): it is read before the term and nothing else of the step reads it.
// With the scales of a pndf_project_options7 (`len`) the term is pndf_fk_len_energy_grad on the row of the pose's group, and `hs` [S] takes
// d E / d sigma of this frame; the scales step in len_step_cpu once every frame of the step has read them.
// With the views of a pndf_project_options8 (`vw`) the term is pndf_fk_views_energy_grad: targets [V][K][2] and confidences [V][K] per pose,
// with the scales or without.  With the trajectory of a pndf_project_options9 (`tr`) the root is read from tr->src and its step
// (pndf_fk_root_smooth_step) goes to tr->dst.  With the moving cameras of a pndf_project_options10 (`pv`) the term is
// pndf_fk_cams_energy_grad on the block of the pose.
static float keypoint_grad_cpu(const PndfKeypoints& kp, const KeypointTables& tb, const int* parent, int nj, const float* q, int64_t pose,
                               float* gk, const PndfCameraTerm& cam = PndfCameraTerm(), float dist = 0.f, float tol = 0.f,
                               const PndfLengths& len = PndfLengths(), float* hs = nullptr, const PndfViews& vw = PndfViews(),
                               const RootTrack* tr = nullptr, const PndfPoseViews& pv = PndfPoseViews()) {
    float W[PNDF_FK_ROWS * MAXJ + PNDF_MAX_SCALES];
    float E;
    if (pv.any()) {
        float root[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, groot[7];
        float* rt = cam.root ? cam.root + pose * 7 : nullptr;
        if (rt) memcpy(root, tr ? tr->src + pose * 7 : rt, sizeof(root));
        E = pndf_fk_cams_energy_grad(q, nj, parent, tb.rest, kp.K, tb.kpj, tb.kpo, kp.target + pose * pv.V * kp.K * 2,
                                     kp.conf ? kp.conf + pose * pv.V * kp.K : nullptr, rt != nullptr, root, cam.rho, pv.V, pv.block(pose),
                                     len.any() ? len.scale + (pose / len.group) * len.S : nullptr, groot, W, 1);
        root_step_cpu(cam, rt, root, groot, dist, tol, pose, tr);
        if (len.any())
            for (int i = 0; i < len.S; ++i) hs[i] = W[pndf_fk_len_row(nj, i)];
    } else if (vw.any()) {
        float root[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, groot[7];
        float* rt = cam.root ? cam.root + pose * 7 : nullptr;
        if (rt) memcpy(root, tr ? tr->src + pose * 7 : rt, sizeof(root));
        E = pndf_fk_views_energy_grad(q, nj, parent, tb.rest, kp.K, tb.kpj, tb.kpo, kp.target + pose * vw.V * kp.K * 2,
                                      kp.conf ? kp.conf + pose * vw.V * kp.K : nullptr, rt != nullptr, root, cam.rho, vw.V, vw.table,
                                      len.any() ? len.scale + (pose / len.group) * len.S : nullptr, groot, W, 1);
        root_step_cpu(cam, rt, root, groot, dist, tol, pose, tr);
        if (len.any())
            for (int i = 0; i < len.S; ++i) hs[i] = W[pndf_fk_len_row(nj, i)];
    } else if (len.any()) {
        const PndfFkCamera fc{cam.fx, cam.fy, cam.cx, cam.cy, cam.rho, cam.image ? 1 : 0};
        float root[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, groot[7];
        float* rt = cam.root ? cam.root + pose * 7 : nullptr;
        if (rt) memcpy(root, tr ? tr->src + pose * 7 : rt, sizeof(root));
        E = pndf_fk_len_energy_grad(q, nj, parent, tb.rest, kp.K, tb.kpj, tb.kpo, kp.target + pose * kp.K * kp.dims,
                                    kp.conf ? kp.conf + pose * kp.K : nullptr, rt != nullptr, root, fc,
                                    len.scale + (pose / len.group) * len.S, groot, W, 1);
        root_step_cpu(cam, rt, root, groot, dist, tol, pose, tr);
        for (int i = 0; i < len.S; ++i) hs[i] = W[pndf_fk_len_row(nj, i)];
    } else if (cam.any()) {
        const PndfFkCamera fc{cam.fx, cam.fy, cam.cx, cam.cy, cam.rho, cam.image ? 1 : 0};
        float root[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, groot[7];
        float* rt = cam.root ? cam.root + pose * 7 : nullptr;
        if (rt) memcpy(root, tr ? tr->src + pose * 7 : rt, sizeof(root));
        E = pndf_fk_camera_energy_grad(q, nj, parent, tb.rest, kp.K, tb.kpj, tb.kpo, kp.target + pose * kp.K * kp.dims,
                                       kp.conf ? kp.conf + pose * kp.K : nullptr, rt != nullptr, root, fc, groot, W, 1);
        root_step_cpu(cam, rt, root, groot, dist, tol, pose, tr);
    } else {
        E = pndf_fk_energy_grad(q, nj, parent, tb.rest, kp.K, tb.kpj, tb.kpo, kp.target + pose * kp.K * 3,
                                kp.conf ? kp.conf + pose * kp.K : nullptr, W, 1);
    }
    for (int j = 0; j < nj; ++j)
        for (int c = 0; c < 4; ++c) gk[4 * j + c] = W[pndf_fk_grad_row(nj, j) + c];
    return E;
}

// The step of the scales of group g (pndf_fk.h: pndf_fk_len_group_sum, pndf_fk_len_step): hs [n][S] the rows its n frames left, dd [n]
// their distances
static void len_step_cpu(const PndfLengths& len, int64_t g, const float* hs, const float* dd, float tol) {
    const int64_t n = len.group;
    bool rests = tol > 0.f;
    for (int64_t f = 0; f < n && rests; ++f) rests = dd[f] < tol;
    float* row = len.scale + g * len.S;
    for (int i = 0; i < len.S; ++i) {
        const float w = len.nu_len * len.rate[i];
        const float H = pndf_fk_len_group_sum(hs + i, len.S, n);
        const float v = pndf_fk_len_step(row[i], H, n, w, len.kappa, len.len_min, len.len_max, rests);
        if (w > 0.f && !rests) row[i] = v;
    }
}

// `gk` (null: none): d E / d Q of the pose's keypoint term of a pndf_project_options5, `nu` its weight: then the step is pndf_fk.h's
// pndf_fit_quat.
static void project_step_cpu(float* q, const float* dq, float d, const pndf_project_options& o, uint32_t held, int nj,
                             const float* anchor = nullptr, const float* conf = nullptr, float mu = 0.f, const float* gk = nullptr,
                             float nu = 0.f) {
    if (o.tol > 0.f && d < o.tol) return;
    for (int j = 0; j < nj; ++j) {
        if ((held >> j) & 1u) continue;
        float u[4];
        if (gk) {
            const float w = !anchor ? 0.f : conf ? mu * conf[j] : mu;
            (void)pndf_fit_quat(q + 4 * j, dq + 4 * j, d, nullptr, nullptr, 0, 0.f, anchor ? anchor + 4 * j : nullptr, w, gk + 4 * j, nu, o.step_size,
                                o.tol, (int)o.renorm, u);
        } else if (anchor) {
            const float w = conf ? mu * conf[j] : mu;
            (void)pndf_denoise_quat(q + 4 * j, dq + 4 * j, d, nullptr, nullptr, 0, 0.f, anchor + 4 * j, w, o.step_size, o.tol, (int)o.renorm, u);
        } else {
            (void)pndf_step_quat(q + 4 * j, dq + 4 * j, d, o.step_size, o.tol, (int)o.renorm, u);
        }
        memcpy(q + 4 * j, u, sizeof(u));
    }
}

// The loop of pndf_project_ex_cpu and pndf_complete_cpu (validated arguments): `steps` times forward + gradient and the step, block by
// block; `observed` null = no joint held; `data`: the observation of a pndf_project_options4 (none: the step without a data term).
static int project_loop_cpu(pndf_cpu_handle h, const float* q_in, const uint32_t* observed, float* q_out, float* d_last, int64_t B,
                            int steps, const pndf_project_options& o, const PndfData& data = PndfData(),
                            const PndfKeypoints& kp = PndfKeypoints(), const PndfCameraTerm& cam = PndfCameraTerm(),
                            const PndfLengths& len = PndfLengths(), const PndfViews& vw = PndfViews(),
                            const PndfRootSmooth& rs = PndfRootSmooth(), const PndfPoseViews& pv = PndfPoseViews()) {
    const int NQ = h->nq();
    // without tracks no pose reads another's root (only the data term of a pndf_project_options9 is possible): its step is in place
    const RootTrack rtk{&rs, cam.root, cam.root, 0};
    const RootTrack* tr = rs.any() ? &rtk : nullptr;
    KeypointTables tb;
    if (kp.any()) pndf_fill_keypoint_tables(tb, kp, h->net.nj);
    return guarded(h, [&] {
    parallel_blocks(B, [&](int64_t p0, int nb, Scratch& S) {
        float qb[PB * 4 * MAXJ], dqb[PB * 4 * MAXJ], dd[PB], ee[PB], gk[4 * MAXJ], hs[PNDF_MAX_SCALES];
        memcpy(qb, q_in + p0 * NQ, sizeof(float) * nb * NQ);
        for (int p = 0; p < nb; ++p) dd[p] = ee[p] = 0.f;
        for (int s = 0; s < steps; ++s) {
            forward_grad_block(*h, qb, nb, nullptr, dd, dqb, true, S);
            for (int p = 0; p < nb; ++p) {
                if (kp.any()) ee[p] = keypoint_grad_cpu(kp, tb, h->net.parent, h->net.nj, qb + p * NQ, p0 + p, gk, cam, dd[p], o.tol, len, hs, vw, tr, pv);
                if (len.moves()) len_step_cpu(len, p0 + p, hs, dd + p, o.tol);      // (without tracks every pose is its own group)
                project_step_cpu(qb + p * NQ, dqb + p * NQ, dd[p], o, observed ? observed[p0 + p] : 0u, h->net.nj,
                                 data.anchor ? data.anchor + (p0 + p) * NQ : nullptr, data.conf ? data.conf + (p0 + p) * h->net.nj : nullptr, data.mu,
                                 kp.any() ? gk : nullptr, kp.nu);
            }
        }
        memcpy(q_out + p0 * NQ, qb, sizeof(float) * nb * NQ);
        if (d_last) memcpy(d_last + p0, dd, sizeof(float) * nb);
        if (kp.energy) memcpy(kp.energy + p0, ee, sizeof(float) * nb);
    });
    });
}

// Host twin of pndf_complete (include/posendf_amd_completion.h): the loop of pndf_project_ex_cpu with the observed joints held.  With
// the default options the step is pndf_project_cpu's (step_size 1 makes its product exact), so with no joint held this is
// pndf_project_ex_cpu bit for bit, defaults included.
extern "C" int pndf_complete_cpu(pndf_cpu_handle h, const float* q_in, const uint32_t* observed, float* q_out, float* d_last,
                                 int64_t B, int steps, const pndf_project_options* opt) {
    if (!h) return PNDF_ERR_BAD_ARG;
    if (!h->smpl) return pndf_fail(h, PNDF_ERR_UNSUPPORTED, SMPL_ONLY);
    pndf_project_options o;
    if (const char* why = pndf_check_project_options(opt, o)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (int rc = check(h, q_in, B)) return rc;
    if (steps < 0 || (B > 0 && !q_out)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative step count or null output pointer");
    if (((uintptr_t)q_in | (uintptr_t)q_out | (uintptr_t)d_last | (uintptr_t)observed) & 3)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned pose, distance or mask buffer");
    return project_loop_cpu(h, q_in, observed, q_out, d_last, B, steps, o);
}

// The whole-track loop of pndf_interpolate_cpu and of pndf_project_ex_cpu with the tracks of a pndf_project_options3 (validated
// arguments), for the handle's joint count: the fill and the band step of pndf_interp.h -- the statements the device kernels run --
// around pndf_forward_grad_cpu.  A step reads the neighbour frames of the track as they were before it (out of place, like the
// device), so the whole track takes one step at a time.  `fill` PNDF_TRACK_GIVEN: `a` is the track [P*T] itself (`b` is not read);
// otherwise pair p is the poses a + p * a_stride and b + p * b_stride.  With lambda == 0 this is project_loop_cpu on the filled
// track with the end frames held, bit for bit.  `data`: the observation and the free end frames of a pndf_project_options4 (motion
// denoising; none: the band step, which pndf_denoise_quat is for an interior frame without a data term).
static int track_loop_cpu(pndf_cpu_handle h, const float* a, int64_t a_stride, const float* b, int64_t b_stride, int fill,
                          const uint32_t* observed, float* track_out, float* d_last, int64_t P, int32_t T, int steps, float lambda,
                          const pndf_project_options& o, const PndfData& data = PndfData(), const PndfKeypoints& kp = PndfKeypoints(),
                          const PndfCameraTerm& cam = PndfCameraTerm(), const PndfLengths& len = PndfLengths(),
                          const PndfViews& vw = PndfViews(), const PndfRootSmooth& rs = PndfRootSmooth(),
                          const PndfPoseViews& pv = PndfPoseViews()) {
    const int nj = h->net.nj;
    const int64_t nq = h->nq(), B = P * T;
    int rc = PNDF_OK;
    KeypointTables tb;
    if (kp.any()) pndf_fill_keypoint_tables(tb, kp, nj);
    const int grc = guarded(h, [&] {
        std::vector<float> other((size_t)(B * nq)), dq(steps ? (size_t)(B * nq) : 0), dd((size_t)B, 0.f), ee((size_t)B, 0.f);
        std::vector<float> hs(len.any() ? (size_t)(B * len.S) : 0);      // d E / d sigma of every frame of the step
        std::vector<float> root2(rs.any() ? (size_t)(B * 7) : 0);      // the second root buffer of a pndf_project_options9: the step is Jacobi
        RootTrack rtk{&rs, cam.root, root2.data(), T};                 // step s reads the caller's root when s is even
        float* cur = (steps & 1) ? other.data() : track_out;      // `steps` swaps later the track is in track_out
        float* nxt = (steps & 1) ? track_out : other.data();
        if (fill == PNDF_TRACK_GIVEN) memcpy(cur, a, sizeof(float) * (size_t)(B * nq));
        else
            for (int64_t p = 0; p < P; ++p)
                for (int j = 0; j < nj; ++j) {
                    const float *A = a + p * a_stride + j * 4, *Bq = b + p * b_stride + j * 4;
                    float bp[4];
                    pndf_quat_align(A, Bq, bp);
                    memcpy(cur + ((p * T) * nj + j) * 4, A, sizeof(float) * 4);
                    memcpy(cur + ((p * T + T - 1) * nj + j) * 4, bp, sizeof(float) * 4);
                    for (int k = 1; k < T - 1; ++k)
                        pndf_interp_fill_quat(A, bp, (float)k / (float)(T - 1), fill == PNDF_TRACK_SLERP ? PNDF_INTERP_SLERP : PNDF_INTERP_NLERP,
                                              cur + ((p * T + k) * nj + j) * 4);
                }
        for (int s = 0; s < steps && rc == PNDF_OK; ++s) {
            rc = pndf_forward_grad_cpu(h, cur, nullptr, dd.data(), dq.data(), B);
            if (rc != PNDF_OK) break;
            for (int64_t f = 0; f < B; ++f) {
                const int k = (int)(f % T);
                const int nbr = (k > 0 ? 1 : 0) | (k < T - 1 ? 2 : 0);
                const uint32_t held = (nbr != 3 && !data.free_ends) ? ~0u : (observed ? observed[f] : 0u);
                float gk[4 * MAXJ];
                if (kp.any()) ee[f] = keypoint_grad_cpu(kp, tb, h->net.parent, nj, cur + f * nq, f, gk, cam, dd[f], o.tol, len,
                                                        len.any() ? hs.data() + f * len.S : nullptr, vw, rs.any() ? &rtk : nullptr, pv);
                for (int j = 0; j < nj; ++j) {
                    const int64_t i = (f * nj + j) * 4;
                    float u[4];
                    const float w = !data.anchor ? 0.f : data.conf ? data.mu * data.conf[f * nj + j] : data.mu;
                    const float *nm = (nbr & 1) ? cur + i - nq : nullptr, *np = (nbr & 2) ? cur + i + nq : nullptr;
                    const float* A = data.anchor ? data.anchor + i : nullptr;
                    if (((held >> j) & 1u) ||
                        (kp.any() ? pndf_fit_quat(cur + i, dq.data() + i, dd[f], nm, np, nbr, lambda, A, w, gk + 4 * j, kp.nu, o.step_size, o.tol, (int)o.renorm, u)
                                  : pndf_denoise_quat(cur + i, dq.data() + i, dd[f], nm, np, nbr, lambda, A, w, o.step_size, o.tol, (int)o.renorm, u)))
                        memcpy(nxt + i, cur + i, sizeof(float) * 4);
                    else
                        memcpy(nxt + i, u, sizeof(float) * 4);
                }
            }
            if (len.moves())      // Jacobi: every frame of this step has read the scales as the step before left them
                for (int64_t g = 0; g < B / len.group; ++g)
                    len_step_cpu(len, g, hs.data() + g * len.group * len.S, dd.data() + g * len.group, o.tol);
            std::swap(cur, nxt);
            if (rs.any()) {
                const float* was = rtk.src;
                rtk.src = rtk.dst;
                rtk.dst = const_cast<float*>(was);
            }
        }
        if (rc == PNDF_OK && rs.any() && rtk.src != cam.root) memcpy(cam.root, rtk.src, sizeof(float) * (size_t)(B * 7));      // an odd step count
        if (rc == PNDF_OK && d_last) memcpy(d_last, dd.data(), sizeof(float) * B);
        if (rc == PNDF_OK && kp.energy) memcpy(kp.energy, ee.data(), sizeof(float) * B);
    });
    return grc != PNDF_OK ? grc : rc;
}

extern "C" int pndf_project_ex_cpu(pndf_cpu_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps,
                                   const pndf_project_options* opt) {
    if (!h) return PNDF_ERR_BAD_ARG;
    pndf_project_options o;
    const uint32_t* observed;      // a pndf_project_options2 brings the joint mask (host memory): completion for any joint tree
    PndfTracks tracks;             // a pndf_project_options3 the tracks besides: interpolation for any joint tree
    PndfData data;                 // a pndf_project_options4 the observation besides (host memory): motion denoising for any joint tree
    PndfKeypoints kp;              // a pndf_project_options5 the 3D keypoints besides (host memory): keypoint fitting for any joint tree
    PndfCameraTerm cam;            // a pndf_project_options6 the camera and the root besides (host memory): image fitting for any joint tree
    PndfLengths len;               // a pndf_project_options7 the bone lengths besides (host memory): one row of scales per track or per pose
    PndfViews vw;                  // a pndf_project_options8 the views besides (host memory): pixels of the same frame in several cameras
    PndfRootSmooth rs;             // a pndf_project_options9 the root's trajectory besides (host memory): the roots of a track coupled, an anchor
    PndfPoseViews pv;              // a pndf_project_options10 the moving cameras besides (host memory): a view table per pose or per frame
    if (const char* why = pndf_check_project_options10(opt, B, h->net.nj, o, observed, tracks, data, kp, cam, len, vw, rs, pv)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (!tracks.frames && !observed && !data.any() && !kp.any() && !kp.energy && pndf_project_options_plain(o))
        return pndf_project_cpu(h, q_in, q_out, d_last, B, steps);
    if (int rc = check(h, q_in, B)) return rc;
    if (steps < 0 || (B > 0 && !q_out)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative step count or null output pointer");
    if (const char* why = pndf_check_observation_apart(data, q_out, B, h->net.nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_keypoints_apart(kp, q_out, B, h->net.nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_root_apart(cam, data, kp, q_in, q_out, B, h->net.nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_lengths_apart(len, cam, data, kp, q_in, q_out, B, h->net.nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_root_anchor_apart(rs, cam, q_out, B, h->net.nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_pose_views_apart(pv, cam, len, q_out, B, h->net.nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (!tracks.frames) return project_loop_cpu(h, q_in, observed, q_out, d_last, B, steps, o, data, kp, cam, len, vw, rs, pv);
    if (B == 0) return PNDF_OK;
    const int64_t nq = h->nq(), T = tracks.frames;
    if ((uintptr_t)q_in < (uintptr_t)(q_out + B * nq) && (uintptr_t)q_out < (uintptr_t)(q_in + B * nq))
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "q_out must not overlap q_in when pndf_project_options3.frames > 0: a step reads the neighbour "
                                              "frames of its input");
    return track_loop_cpu(h, q_in, T * nq, q_in + (T - 1) * nq, T * nq, tracks.fill, observed, q_out, d_last, B / T, (int32_t)T, steps,
                          tracks.lambda, o, data, kp, cam, len, vw, rs, pv);
}

// Host twin of pndf_interpolate (include/posendf_amd_interpolation.h): track_loop_cpu on the 21-joint table; with lambda == 0 this is
// pndf_complete_cpu on the filled track with the end frames observed, bit for bit.  Another skeleton interpolates through
// pndf_project_ex_cpu with a pndf_project_options3.
extern "C" int pndf_interpolate_cpu(pndf_cpu_handle h, const float* a, const float* b, const uint32_t* observed, float* track_out,
                                    float* d_last, int64_t P, int32_t T, int32_t mode, int steps, float lambda,
                                    const pndf_project_options* opt) {
    if (!h) return PNDF_ERR_BAD_ARG;
    if (!h->smpl) return pndf_fail(h, PNDF_ERR_UNSUPPORTED, SMPL_ONLY);
    pndf_project_options o;
    if (const char* why = pndf_check_project_options(opt, o)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_interp_check_mode(mode)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_interp_check_lambda(lambda)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (!h->have_weights) return pndf_fail(h, PNDF_ERR_NO_WEIGHTS, "pndf_cpu_load_weights has not been called");
    if (steps < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative step count");
    if (const char* why = pndf_interp_check_shape(P, T)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (P == 0) return PNDF_OK;
    if (!a || !b || !track_out) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pose / output pointer");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)track_out | (uintptr_t)d_last | (uintptr_t)observed) & 3)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned pose, distance or mask buffer");
    return track_loop_cpu(h, a, NQ, b, NQ, mode == PNDF_INTERP_SLERP ? PNDF_TRACK_SLERP : PNDF_TRACK_NLERP, observed, track_out, d_last, P, T,
                          steps, lambda, o);
}

// ---- host twin of pndf_second_order (include/posendf_amd_second_order.h): d, g = grad_q d, t = <v, g> and w_d g + w_t H v, one pose at
// a time through the dual-number network (csrc/pndf_second_order.hip has the derivation): primal and tangent forward with sigma'
// and sigma'' kept, then both adjoint chains in one reverse -- the tangent's (the first-order reverse, seed 1) and the primal's
// (seed 0, zbar = abar sigma' + adotbar zdot sigma'') --, then the normalisation with its curvature term.  Values are stored in
// fp32; a dot product is summed in double and rounded once.
namespace {

void act3(const Act& a, bool output_layer, float z, float& y, float& d1, float& d2) {
    if (a.kind == PNDF_ACT_SOFTPLUS) {
        const float bz = z * a.beta;
        if (bz > 20.0f) {
            y = z; d1 = 1.0f; d2 = 0.0f;
        } else {
            const float e = expf(bz);
            y = log1pf(e) / a.beta;
            d1 = e / (e + 1.0f);
            d2 = a.beta * d1 * (1.0f - d1);
        }
        return;
    }
    const float slope = (a.kind == PNDF_ACT_LRELU && !output_layer) ? 0.01f : 0.0f;
    y = z > 0.0f ? z : z * slope;
    d1 = z > 0.0f ? 1.0f : slope;
    d2 = 0.0f;
}

// y = W x (+ b): w [out][in]
void matvec(const float* w, const float* b, int out, int in, const float* x, float* y) {
    for (int o = 0; o < out; ++o) {
        double s = b ? (double)b[o] : 0.0;
        for (int i = 0; i < in; ++i) s += (double)w[(size_t)o * in + i] * (double)x[i];
        y[o] = (float)s;
    }
}

struct SoScratch {
    std::vector<float> a, ad, u, ub, t0, t1, d1[MAXLIN], c2[MAXLIN];
};

void second_order_pose(const pndf_cpu_engine& E, const float* q, const float* v, float wd, float wt, float* d, float* g, float* t,
                       float* out, SoScratch& S) {
    const Act act{E.net.act, E.net.beta};
    const Act eact{E.net.enc_act, E.net.enc_beta};
    constexpr int FIN = 4 + FEAT;
    // ---- normalisation: x, xdot = J_N v
    float s[4], va[4], x[NQ], xd[NQ];
    bool live[4];
    for (int c = 0; c < 4; ++c) {
        double ss = 0.0;
        for (int j = 0; j < NJ; ++j) ss += (double)q[4 * j + c] * (double)q[4 * j + c];
        s[c] = (float)sqrt(ss);
        live[c] = s[c] > 1e-12f;
        const float den = std::max(s[c], 1e-12f);
        double a = 0.0;
        for (int j = 0; j < NJ; ++j) {
            x[4 * j + c] = q[4 * j + c] / den;
            a += (double)x[4 * j + c] * (double)v[4 * j + c];
        }
        va[c] = (float)a;
        for (int j = 0; j < NJ; ++j) xd[4 * j + c] = live[c] ? (v[4 * j + c] - x[4 * j + c] * va[c]) / s[c] : v[4 * j + c] / 1e-12f;
    }
    // ---- encoder: primal and tangent, the derivatives kept per bone
    float feat[NFEAT], tfeat[NFEAT], d1h[NJ][HID], d2h[NJ][HID], hz[NJ][HID], d1o[NJ][FEAT], d2o[NJ][FEAT], oz[NJ][FEAT];
    for (int j = 0; j < NJ; ++j) {
        const int in = enc_in(j);
        float xi[FIN], xdi[FIN], zh[HID], ah[HID], ahd[HID], zo[FEAT];
        memcpy(xi, x + 4 * j, sizeof(float) * 4);
        memcpy(xdi, xd + 4 * j, sizeof(float) * 4);
        if (PARENT[j] >= 0) {
            memcpy(xi + 4, feat + FEAT * PARENT[j], sizeof(float) * FEAT);
            memcpy(xdi + 4, tfeat + FEAT * PARENT[j], sizeof(float) * FEAT);
        }
        matvec(E.enc[j][0].w.data(), E.enc[j][0].b.data(), HID, in, xi, zh);
        matvec(E.enc[j][0].w.data(), nullptr, HID, in, xdi, hz[j]);
        for (int k = 0; k < HID; ++k) {
            act3(eact, false, zh[k], ah[k], d1h[j][k], d2h[j][k]);
            ahd[k] = d1h[j][k] * hz[j][k];
        }
        matvec(E.enc[j][1].w.data(), E.enc[j][1].b.data(), FEAT, HID, ah, zo);
        matvec(E.enc[j][1].w.data(), nullptr, FEAT, HID, ahd, oz[j]);
        for (int i = 0; i < FEAT; ++i) {
            act3(eact, false, zo[i], feat[FEAT * j + i], d1o[j][i], d2o[j][i]);
            tfeat[FEAT * j + i] = oz[j][i] * d1o[j][i];
        }
    }
    // ---- trunk: primal and tangent; c2 = sigma'' zdot
    const int NL = E.net.L;
    S.a.assign(feat, feat + NFEAT);
    S.ad.assign(tfeat, tfeat + NFEAT);
    for (int l = 0; l < NL; ++l) {
        const Layer& L = E.lin[l];
        S.t0.resize(L.out); S.t1.resize(L.out); S.d1[l].resize(L.out); S.c2[l].resize(L.out);
        matvec(L.w.data(), L.b.data(), L.out, L.in, S.a.data(), S.t0.data());
        matvec(L.w.data(), nullptr, L.out, L.in, S.ad.data(), S.t1.data());
        for (int o = 0; o < L.out; ++o) {
            float y, d2;
            act3(act, l == NL - 1, S.t0[o], y, S.d1[l][o], d2);
            S.t0[o] = y;
            S.c2[l][o] = d2 * S.t1[o];
            S.t1[o] = S.d1[l][o] * S.t1[o];
        }
        S.a.swap(S.t0);
        S.ad.swap(S.t1);
    }
    if (d) *d = S.a[0];
    // ---- reverse: u = adjoint of the tangent's pre-activation (seed 1), ub = of the primal's (seed 0)
    S.u.assign(1, S.d1[NL - 1][0]);
    S.ub.assign(1, S.c2[NL - 1][0]);
    for (int l = NL - 1; l >= 0; --l) {
        const Layer& L = E.lin[l];
        S.t0.resize(L.in); S.t1.resize(L.in);
        matvec(L.wt.data(), nullptr, L.in, L.out, S.u.data(), S.t0.data());
        matvec(L.wt.data(), nullptr, L.in, L.out, S.ub.data(), S.t1.data());
        if (l > 0)
            for (int i = 0; i < L.in; ++i) {
                S.t1[i] = S.t1[i] * S.d1[l - 1][i] + S.t0[i] * S.c2[l - 1][i];
                S.t0[i] = S.t0[i] * S.d1[l - 1][i];
            }
        S.u.swap(S.t0);
        S.ub.swap(S.t1);
    }
    // ---- encoder reverse, children before parents: gx = d d / d x, xb = hess f xdot
    float gx[NQ], xb[NQ];
    float* gf = S.u.data();
    float* af = S.ub.data();
    for (int j = NJ - 1; j >= 0; --j) {
        const int in = enc_in(j);
        float zob[FEAT], zodb[FEAT], sb[HID], sdb[HID], zhb[HID], zhdb[HID], gi[FIN], ai[FIN];
        for (int i = 0; i < FEAT; ++i) {
            zodb[i] = gf[FEAT * j + i] * d1o[j][i];
            zob[i] = af[FEAT * j + i] * d1o[j][i] + gf[FEAT * j + i] * oz[j][i] * d2o[j][i];
        }
        matvec(E.enc[j][1].wt.data(), nullptr, HID, FEAT, zodb, sdb);
        matvec(E.enc[j][1].wt.data(), nullptr, HID, FEAT, zob, sb);
        for (int k = 0; k < HID; ++k) {
            zhb[k] = sb[k] * d1h[j][k] + sdb[k] * hz[j][k] * d2h[j][k];
            zhdb[k] = sdb[k] * d1h[j][k];
        }
        matvec(E.enc[j][0].wt.data(), nullptr, in, HID, zhdb, gi);
        matvec(E.enc[j][0].wt.data(), nullptr, in, HID, zhb, ai);
        memcpy(gx + 4 * j, gi, sizeof(float) * 4);
        memcpy(xb + 4 * j, ai, sizeof(float) * 4);
        if (PARENT[j] >= 0)
            for (int i = 0; i < FEAT; ++i) {
                gf[FEAT * PARENT[j] + i] += gi[4 + i];
                af[FEAT * PARENT[j] + i] += ai[4 + i];
            }
    }
    // ---- the normalisation: per component column with n = x, p = xdot, g = J g_x:  H v = J xbar - [(g_x . p) n + (n . v) g + (g_x . n) p] / s;
    // on the clamp J = I / eps and there is no curvature
    double tt = 0.0;
    for (int c = 0; c < 4; ++c) {
        double b = 0.0, e = 0.0, gp = 0.0;
        for (int j = 0; j < NJ; ++j) {
            b += (double)x[4 * j + c] * (double)gx[4 * j + c];
            e += (double)x[4 * j + c] * (double)xb[4 * j + c];
            gp += (double)gx[4 * j + c] * (double)xd[4 * j + c];
        }
        const float bf = (float)b, ef = (float)e, gpf = (float)gp;
        for (int j = 0; j < NJ; ++j) {
            const int i = 4 * j + c;
            float gg, hv;
            if (live[c]) {
                gg = (gx[i] - x[i] * bf) / s[c];
                hv = (xb[i] - x[i] * ef) / s[c] - (gpf * x[i] + va[c] * gg + bf * xd[i]) / s[c];
            } else {
                gg = gx[i] / 1e-12f;
                hv = xb[i] / 1e-12f;
            }
            tt += (double)v[i] * (double)gg;
            if (g) g[i] = gg;
            if (out) out[i] = wd * gg + wt * hv;
        }
    }
    if (t) *t = (float)tt;
}

}  // namespace

extern "C" int pndf_second_order_cpu(pndf_cpu_handle h, const float* q, const float* v, const float* w_d, const float* w_t, float* d,
                                     float* g, float* t, float* out, int64_t B) {
    if (!h) return PNDF_ERR_BAD_ARG;
    if (!h->smpl) return pndf_fail(h, PNDF_ERR_UNSUPPORTED, SMPL_ONLY);
    if (!h->net.encoder)
        return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "the second order needs the structure encoder (model.StrEnc.use: True, dims[0] = 126)");
    if (int rc = check(h, q, B)) return rc;
    if (B == 0) return PNDF_OK;
    if (!v) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null direction pointer");
    if (((uintptr_t)q | (uintptr_t)v | (uintptr_t)w_d | (uintptr_t)w_t | (uintptr_t)d | (uintptr_t)g | (uintptr_t)t | (uintptr_t)out) & 3)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned pose, direction, weight or output buffer");
    auto overlaps = [B](const float* a, const float* b) {
        return a && b && (uintptr_t)a < (uintptr_t)(b + B * NQ) && (uintptr_t)b < (uintptr_t)(a + B * NQ);
    };
    if (overlaps(out, q) || overlaps(out, v) || overlaps(g, q) || overlaps(g, v) || overlaps(g, out))
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "out and g must not alias q, v or each other");
    return guarded(h, [&] {
        parallel_blocks(B, [&](int64_t p0, int nb, Scratch&) {
            SoScratch S;
            for (int64_t p = p0; p < p0 + nb; ++p)
                second_order_pose(*h, q + p * NQ, v + p * NQ, w_d ? w_d[p] : 0.0f, w_t ? w_t[p] : 1.0f, d ? d + p : nullptr,
                                  g ? g + p * NQ : nullptr, t ? t + p : nullptr, out ? out + p * NQ : nullptr, S);
        });
    });
}

// ------------------------------------------------------------------ online training data (include/posendf_amd_online.h)
// The sampler's host side: the default options, the thresholds of a list of shares, and the host twin of pndf_online_sample --
// pndf_online.h's expression, pose by pose on the calling thread (84 floats and 22 Philox blocks per 21-joint pose: meant for small pools
// and for holding the kernel to).  No handle: a refusal's text goes to the slot of pndf_cpu_last_error(NULL).
namespace {

int online_fail(int code, const std::string& msg) { return pndf_fail<pndf_cpu_engine>(nullptr, code, msg); }

}  // namespace

extern "C" int pndf_online_shares(pndf_online_opts* opt, const float* shares) {
    if (!opt) return online_fail(PNDF_ERR_BAD_ARG, "pndf_online_shares: opt is null");
    uint32_t cum[PNDF_ONLINE_MAX_SIGMA];
    if (const char* why = pndf_online_thresholds(opt->n_sigma, shares, cum)) return online_fail(PNDF_ERR_BAD_ARG, std::string("pndf_online_shares: ") + why);
    for (int g = 0; g < PNDF_ONLINE_MAX_SIGMA; ++g) opt->cum[g] = g < opt->n_sigma ? cum[g] : 0xffffffffu;
    return PNDF_OK;
}

extern "C" int pndf_online_default_opts(pndf_online_opts* opt) {
    if (!opt) return online_fail(PNDF_ERR_BAD_ARG, "pndf_online_default_opts: opt is null");
    memset(opt, 0, sizeof(*opt));
    const float sigma[5] = {0.01f, 0.05f, 0.1f, 0.25f, 0.5f}, shares[5] = {0.2f, 0.2f, 0.2f, 0.2f, 0.2f};      // create_data.py:51-52
    opt->noise = PNDF_ONLINE_UNIFORM;
    opt->n_sigma = 5;
    for (int g = 0; g < 5; ++g) opt->sigma[g] = sigma[g];
    return pndf_online_shares(opt, shares);
}

// `name`: the entry point, for the texts; J floats x 4 and 1 + J Philox blocks per pose
static int online_sample_cpu(const char* name, const float* man_db, int64_t N, int J, int64_t first, int64_t count, const pndf_online_opts* opt,
                             float* q, int64_t* src, int32_t* group) {
    if (const char* why = pndf_online_check(man_db, N, J, first, count, opt, q, src, group, 4))
        return online_fail(PNDF_ERR_BAD_ARG, std::string(name) + ": " + why);
    for (int64_t p = 0; p < count; ++p) {
        const int64_t i = first + p;
        int64_t row;
        int32_t g;
        float sigma;
        pndf_online_pick(*opt, i, N, &row, &g, &sigma);
        for (int j = 0; j < J; ++j)
            pndf_online_quat(opt->seed, opt->draw, i, j, opt->noise, sigma, man_db + (row * J + j) * 4, q + (p * J + j) * 4);
        if (src) src[p] = row;
        if (group) group[p] = g;
    }
    return PNDF_OK;
}

extern "C" int pndf_online_sample_cpu(const float* man_db, int64_t N, int64_t first, int64_t count, const pndf_online_opts* opt, float* q,
                                      int64_t* src, int32_t* group) {
    return online_sample_cpu("pndf_online_sample_cpu", man_db, N, NJ, first, count, opt, q, src, group);
}

// include/posendf_amd_skeleton_data.h
extern "C" int pndf_skel_online_sample_cpu(const float* man_db, int64_t N, int32_t num_joints, int64_t first, int64_t count,
                                           const pndf_online_opts* opt, float* q, int64_t* src, int32_t* group) {
    return online_sample_cpu("pndf_skel_online_sample_cpu", man_db, N, num_joints, first, count, opt, q, src, group);
}
