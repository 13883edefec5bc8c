// fuse_host_check.cpp - extractorb_amd/csrc/k_fuse.hip compiled for the HOST (tests/cpp/host_shim/hip/hip_runtime.h stands in for the device
// vocabulary) and run one thread at a time.  Two uses, both without a GPU:
//   * as a shared library (tests/test_fuse.py): fuse_host() over the scenes of the GPU tests, compared with the walk - the kernel's own
//     arithmetic and control flow, not a restatement of it;
//   * as a stand-alone program under -fsanitize=address,undefined: exact-size heap buffers, valid and CORRUPT grids (garbage offsets and
//     indices, counts above the capacities, octaves outside the tables), a negative radius - every access of the kernel stays inside its arrays.
// d_n_fused is not emulated (a wave is one lane in the shim).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_fuse.hip"

using namespace orbx;
extern "C" int orbx_predict_scale_breakpoints(float, int, float*);

static void runAll(const float* w, const float* nv, const float* dist, const uint8_t* md, const int* nmp, const uint8_t* fl, const float* poses,
                   const Keypoint* kps, const float* ur, const uint8_t* desc, const int* nout, const int* off, const int* idx, const FuseParams& p,
                   int* bi, int* bd, uint8_t* ex, int* nf, int pairs) {
    for (int pr = 0; pr < pairs; pr++)
        for (int b = 0; b < (p.mpCapacity + 255) / 256; b++)
            for (int t = 0; t < 256; t++) {
                blockIdx = dim3(b, pr); threadIdx = dim3(t);
                k_fuse(w, nv, dist, md, nmp, fl, poses, kps, ur, desc, nout, off, idx, p, bi, bd, ex, nf);
            }
}

extern "C" int fuse_host_params_size() { return (int)sizeof(FuseParams); }
extern "C" void fuse_host(const float* w, const float* nv, const float* dist, const uint8_t* md, const int* nmp, const uint8_t* fl, const float* poses,
                          const void* kps, const float* ur, const uint8_t* desc, const int* nout, const int* off, const int* idx, const void* params,
                          int* bi, int* bd, uint8_t* ex, int* nf, int pairs) {
    runAll(w, nv, dist, md, nmp, fl, poses, (const Keypoint*)kps, ur, desc, nout, off, idx, *(const FuseParams*)params, bi, bd, ex, nf, pairs);
}

#ifdef FUSE_HOST_MAIN
int main() {
    std::mt19937 rng(7);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int trial = 0; trial < 6; trial++) {
        const bool corrupt = trial >= 3;
        const int cap = trial % 3 == 0 ? 97 : 1302, mpCap = trial % 3 == 1 ? 5000 : 333, pairs = 3, B = 3;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<Keypoint> kps((size_t)B * cap);
        std::vector<uint8_t> desc((size_t)B * cap * 32);
        std::vector<float> ur((size_t)B * cap), poses(B * 12, 0.f);
        std::vector<int> nout(B), off((size_t)B * 3073), idx((size_t)B * cap);
        for (int f = 0; f < B; f++) {
            nout[f] = corrupt ? cap + 50 : cap - 5;
            poses[f * 12 + 0] = poses[f * 12 + 5] = poses[f * 12 + 10] = 1.f; poses[f * 12 + 3] = U(-.2f, .2f);
            std::vector<std::vector<int>> cells(64 * 48);
            for (int i = 0; i < cap; i++) {
                Keypoint& k = kps[(size_t)f * cap + i];
                k.x = U(0, 634); k.y = U(0, 474); k.octave = corrupt ? (int)U(-3, 20) : (int)U(0, 8);
                ur[(size_t)f * cap + i] = U(0, 1) < .5f ? k.x - 5 : -1.f;
                if (i < cap - 5) cells[(int)std::round(k.x * .1f) * 48 + (int)std::round(k.y * .1f)].push_back(i);
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
            const float z = U(-1, 8), u = U(-50, 700), v = U(-50, 530);
            w[3 * i] = (u - 320) / 450 * z; w[3 * i + 1] = (v - 240) / 450 * z; w[3 * i + 2] = z;
            const float d = std::sqrt(w[3 * i] * w[3 * i] + w[3 * i + 1] * w[3 * i + 1] + z * z);
            for (int c = 0; c < 3; c++) nv[3 * i + c] = w[3 * i + c] / (d + 1e-6f);
            dist[3 * i] = 0; dist[3 * i + 1] = 1e9f; dist[3 * i + 2] = d * U(0.5f, corrupt ? 1e30f : 4.f);
        }
        for (auto& d : md) d = (uint8_t)rng();
        for (auto& x : fl) x = rng() % 8 != 0;
        std::vector<int> nmp(1, corrupt ? mpCap + 9 : mpCap - 3), bi((size_t)pairs * mpCap), bd((size_t)pairs * mpCap), nf(pairs, 0);
        std::vector<uint8_t> ex((size_t)pairs * mpCap);
        FuseParams p{};
        p.fx = p.fy = 450; p.cx = 320; p.cy = 240; p.minX = 0; p.maxX = 640; p.minY = 0; p.maxY = 480; p.wInv = 0.1f; p.hInv = 0.1f;
        p.nlevels = 8;
        for (int l = 0; l < 8; l++) { p.scale[l] = std::pow(1.2f, (float)l); p.invSigma2[l] = 1 / (p.scale[l] * p.scale[l]); }
        orbx_predict_scale_breakpoints(1.2f, 8, p.breaks);
        p.mbf = 40; p.th = trial == 2 ? -300.f : (corrupt ? 40.f : 3.f); p.thLow = 50; p.reprojCheck = trial & 1; p.capacity = cap; p.mpCapacity = mpCap;
        p.kfFirst = 0; p.kfStep = 1; p.mpFirst = 0; p.mpStep = 0;
        runAll(w.data(), nv.data(), dist.data(), md.data(), nmp.data(), fl.data(), poses.data(), kps.data(), trial == 4 ? nullptr : ur.data(), desc.data(),
               nout.data(), off.data(), idx.data(), p, bi.data(), bd.data(), ex.data(), nf.data(), pairs);
        long hist[8] = {};
        for (uint8_t e : ex) hist[e & 7]++;
        std::printf("trial %d capacity %d mappoints %d corrupt %d exits", trial, cap, mpCap, (int)corrupt);
        for (long h : hist) std::printf(" %ld", h);
        std::printf("\n");
    }
    std::printf("clean\n");
    return 0;
}
#endif
