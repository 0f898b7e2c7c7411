// triangulate_internal.h -- the triangulation kernel of csrc/triangulate.hip as the keyframe handles (csrc/keyframe.hip) enqueue it behind their search
#pragma once
#include "common.h"

namespace eao {
namespace tri {

constexpr int kMaxProb = 16;      // neighbours per launch: their records travel in the kernel arguments

struct Side {      // what the loop reads of one keyframe: device-readable addresses
    int n, nlevels;
    const float* kx; const float* ky; const float* ur; const float* depth; const float* rawx; const float* rawy;
    const int* oct;
    const float* sf; const float* s2;
};
struct Prob {
    Side K2;
    eao_tri_camera cam2;
    const int* match;      // K1.n slots: index into K2 or -1
};

// Enqueues the kernel for nProb <= kMaxProb neighbours on `s`: verdict / x3d rows of K1.n slots per neighbour, from the given bases.  No wait.
void launch(hipStream_t s, const Side& K1, const eao_tri_camera& cam1, float ratioFactor, int nProb, const Prob* P, int* verdict, float* x3d);

}  // namespace tri
}  // namespace eao
