// Interface of conv_generic.hip: the generic implicit-GEMM kernels (k_gather_gemm, k_wgrad) behind conv.hip's routes.
#pragma once
#include <hip/hip_runtime.h>

// What conv.hip fills.  The kernels' own parameter types (GemmArgs, WgradArgs) are these, re-declared inside conv_generic.hip's
// anonymous namespace: a type of that namespace cannot appear in a function that two translation units share.
struct GemmProblem {
    const float* A; const float* X; float* Y; const float* bias;
    int M, K;
    int Nb, C, Hi, Wi;
    int NY, NX;
    int sy, oy, da, sx, ox, db;
    int pad_mode;   // 0 zero, 1 reflect
    long out_ns, out_cs;
    int out_w, osy, ooy, osx, oox;
    int act;        // 0 none, 1 relu, 2 elu, 3 sigmoid, 4 tanh
    int in_norm;    // conv1: (x - 0.45) / 0.225 on in-bounds taps (resnet_encoder.py:94)
    int xcd_swizzle;
};

struct WgradProblem {
    const float* dY; const float* X; float* out;   // out: dW (splits == 1) or slabs [splits][M][J]
    int M, J;
    int Nb, C, Hi, Wi;
    int NY, NX;
    int sy, oy, da, sx, ox, db;
    int pad_mode, in_norm;
    long dy_ns, dy_cs;      // dY[n*dy_ns + m*dy_cs + y*NX + x]
    long pix_per_split;
};

int dispatch_gemm(int TA, int TB, const GemmProblem& g, hipStream_t st);
int dispatch_wgrad(int TA, int TB, const WgradProblem& g, int splits, hipStream_t st);
