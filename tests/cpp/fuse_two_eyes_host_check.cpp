// fuse_two_eyes_host_check.cpp - extractorb_amd/csrc/k_fuse_two_eyes.hip compiled for the HOST (tests/cpp/host_shim stands in for the device
// vocabulary; fuse_two_eyes_shim.h brings what this kernel needs beyond k_fuse.hip's) and run one thread at a time: a workgroup is every
// thread's fuseTwoEyesStage into the workgroup's two LDS arrays, then every thread's fuseTwoEyesLane - the two halves of the kernel around its
// one barrier.  Two uses, both without a GPU:
//   * as a shared library (tests/test_fuse_two_eyes.py): fuse_two_eyes_host() over the scenes of the GPU tests, compared with the walk - the
//     kernel's own arithmetic and control flow, not a restatement of it; fuse_two_eyes_bad_eyes() is the entry's predicate on `eyes`;
//   * as a stand-alone program under -fsanitize=address,undefined: exact-size heap buffers, valid and CORRUPT grids (garbage offsets and
//     indices, counts above the capacities, octaves outside the tables), a negative radius, every `eyes` - every access stays inside its arrays.
// d_n_fused is not emulated (a wave is one lane in the shim).
#include "host_shim/fuse_two_eyes_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_fuse_two_eyes.hip"
#include "../../extractorb_amd/csrc/orbx_entry.hpp"

using namespace orbx;
extern "C" int orbx_predict_scale_breakpoints(float, int, float*);

static void runAll(const float* w, const float* nv, const float* dist, const uint8_t* md, const int* nmp, const uint8_t* fl, const float* poses,
                   const Keypoint* kps, const uint8_t* desc, const int* nout, const int* off, const int* idx, const FuseTwoEyesParams& p, int* bi,
                   int* bd, uint8_t* ex, int* nf, int pairs) {
    for (int pr = 0; pr < pairs; pr++)
        for (int b = 0; b < fuseTwoEyesGroups(p.mpCapacity, p.eyes); b++) {
            // exact-size blocks: the sanitized program sees an access past the thirty invariants or the sixteen camera floats
            std::vector<float> sEye(30), sCam(16);
            for (int t = 0; t < 256; t++) {
                blockIdx = dim3(b, pr); threadIdx = dim3(t);
                fuseTwoEyesStage(poses, p, sEye.data(), sCam.data());
            }
            for (int t = 0; t < 256; t++) {
                blockIdx = dim3(b, pr); threadIdx = dim3(t);
                fuseTwoEyesLane(w, nv, dist, md, nmp, fl, kps, desc, nout, off, idx, p, sEye.data(), sCam.data(), bi, bd, ex, nf);
            }
        }
}

extern "C" int fuse_two_eyes_host_params_size() { return (int)sizeof(FuseTwoEyesParams); }
extern "C" int fuse_two_eyes_bad_eyes(int eyes, int reprojCheck) { return badFuseEyes(eyes, reprojCheck) ? 1 : 0; }
extern "C" void fuse_two_eyes_host(const float* w, const float* nv, const float* dist, const uint8_t* md, const int* nmp, const uint8_t* fl,
                                   const float* poses, const void* kps, const uint8_t* desc, const int* nout, const int* off, const int* idx,
                                   const void* params, int* bi, int* bd, uint8_t* ex, int* nf, int pairs) {
    runAll(w, nv, dist, md, nmp, fl, poses, (const Keypoint*)kps, desc, nout, off, idx, *(const FuseTwoEyesParams*)params, bi, bd, ex, nf, pairs);
}
// the thirty invariants of one rig, as the kernel's thirty lanes compute them
extern "C" void fuse_two_eyes_rig(const float* pose12, const float* tlr12, float* out30) {
    for (int j = 0; j < 30; j++) out30[j] = fuseTwoEyesRigElement(pose12, tlr12, j);
}

#ifdef FUSE_TWO_EYES_HOST_MAIN
int main() {
    std::mt19937 rng(11);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int trial = 0; trial < 8; trial++) {
        const bool corrupt = trial >= 4;
        const int cap = trial % 4 == 0 ? 97 : 1302, mpCap = trial % 4 == 1 ? 5000 : 333, pairs = 3, rigs = 3, B = 2 * rigs;
        const int eyes = trial % 4 == 3 ? 1 : trial % 4 == 2 ? 2 : 3;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<Keypoint> kps((size_t)B * cap);
        std::vector<uint8_t> desc((size_t)B * cap * 32);
        std::vector<float> poses(rigs * 12, 0.f);
        std::vector<int> nout(B), off((size_t)B * 3073), idx((size_t)B * cap);
        for (int r = 0; r < rigs; r++) { poses[r * 12 + 0] = poses[r * 12 + 5] = poses[r * 12 + 10] = 1.f; poses[r * 12 + 3] = U(-.2f, .2f); }
        for (int f = 0; f < B; f++) {
            nout[f] = corrupt ? cap + 50 : cap - 5 - (f & 1 ? 0 : 9);      // NRight > NLeft
            std::vector<std::vector<int>> cells(64 * 48);
            for (int i = 0; i < cap; i++) {
                Keypoint& k = kps[(size_t)f * cap + i];
                k.x = U(0, 634); k.y = U(0, 474); k.octave = corrupt ? (int)U(-3, 20) : (int)U(0, 8);
                if (i < cap - 14) cells[(int)std::round(k.x * .1f) * 48 + (int)std::round(k.y * .1f)].push_back(i);
            }
            int s = 0;
            for (int c = 0; c < 64 * 48; c++) { off[(size_t)f * 3073 + c] = s; for (int i : cells[c]) idx[(size_t)f * cap + s++] = i; }
            off[(size_t)f * 3073 + 64 * 48] = s;
            if (corrupt) {
                for (int c = 0; c <= 64 * 48; c++) off[(size_t)f * 3073 + c] = (int)U(-1e6f, 1e6f);
                for (int i = 0; i < cap; i++) idx[(size_t)f * cap + i] = (int)U(-1e6f, 1e6f);
            }
        }
        for (auto& d : desc) d = (uint8_t)rng();
        std::vector<float> w((size_t)mpCap * 3), nv((size_t)mpCap * 3), dist((size_t)mpCap * 3);
        std::vector<uint8_t> md((size_t)mpCap * 32), fl((size_t)pairs * mpCap);
        for (int i = 0; i < mpCap; i++) {
            const float z = U(-1, 8), th = U(0, 1.3f), ps = U(-3.14f, 3.14f);
            w[3 * i] = z * std::tan(th) * std::cos(ps); w[3 * i + 1] = z * std::tan(th) * std::sin(ps); w[3 * i + 2] = i % 50 == 0 ? 0.f : z;
            const float d = std::sqrt(w[3 * i] * w[3 * i] + w[3 * i + 1] * w[3 * i + 1] + w[3 * i + 2] * w[3 * i + 2]);
            for (int c = 0; c < 3; c++) nv[3 * i + c] = w[3 * i + c] / (d + 1e-6f);
            dist[3 * i] = 0; dist[3 * i + 1] = 1e9f; dist[3 * i + 2] = d * U(0.5f, corrupt ? 1e30f : 4.f);
        }
        for (auto& d : md) d = (uint8_t)rng();
        for (auto& x : fl) x = rng() % 8 != 0;
        std::vector<int> nmp(1, corrupt ? mpCap + 9 : mpCap - 3), bi((size_t)pairs * 2 * mpCap), bd((size_t)pairs * 2 * mpCap), nf(pairs * 2, 0);
        std::vector<uint8_t> ex((size_t)pairs * 2 * mpCap, 0);
        FuseTwoEyesParams p{};
        const float camL[8] = {190.f, 190.f, 320.f, 240.f, 0.003f, 0.0007f, -0.002f, 0.0002f}, camR[8] = {188.f, 189.f, 322.f, 238.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < 8; c++) { p.cam[0][c] = camL[c]; p.cam[1][c] = camR[c]; }
        p.minX = 0; p.maxX = 640; p.minY = 0; p.maxY = 480; p.wInv = 0.1f; p.hInv = 0.1f;
        p.tlr[0] = p.tlr[5] = p.tlr[10] = 1.f; p.tlr[3] = 0.1f;
        p.nlevels = 8;
        for (int l = 0; l < 8; l++) { p.scale[l] = std::pow(1.2f, (float)l); p.invSigma2[l] = 1 / (p.scale[l] * p.scale[l]); }
        orbx_predict_scale_breakpoints(1.2f, 8, p.breaks);
        p.th = trial == 2 ? -300.f : (corrupt ? 40.f : 3.f); p.thLow = 50; p.reprojCheck = eyes == 1 ? (trial < 4) : 1; p.eyes = eyes;
        p.capacity = cap; p.mpCapacity = mpCap; p.kfFirst = 0; p.kfStep = 1; p.mpFirst = 0; p.mpStep = 0;
        runAll(w.data(), nv.data(), dist.data(), md.data(), nmp.data(), fl.data(), poses.data(), kps.data(), desc.data(), nout.data(), off.data(),
               idx.data(), p, bi.data(), bd.data(), ex.data(), nf.data(), pairs);
        long hist[8] = {};
        for (uint8_t e : ex) hist[e & 7]++;
        std::printf("trial %d capacity %d mappoints %d corrupt %d eyes %d exits", trial, cap, mpCap, (int)corrupt, eyes);
        for (long h : hist) std::printf(" %ld", h);
        std::printf("\n");
    }
    std::printf("clean\n");
    return 0;
}
#endif
