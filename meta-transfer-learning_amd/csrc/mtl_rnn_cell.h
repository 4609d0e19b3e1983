// The LSTM and GRU cell of one (batch row, hidden unit): the ONE definition of the forward and backward arithmetic that the per-step
// cell kernels and the persistent layer / stack kernels (mtl_lstm.hip, mtl_gru.hip) all call, so the launch modes differ in their
// summation orders only.  Operand order and parenthesisation are part of the contract: the results are compared bit for bit.
//
// Some operands that a per-step kernel reads straight from a tensor are taken by ADDRESS and read where the formula uses them (the
// GRU's previous state after its tanh, for one); a persistent kernel, which holds them in registers, passes the register's address.
// Taken by value those loads move ahead of the transcendental functions and the per-step kernels no longer compile to the code of
// the written-out formulas.  lstm_cell_act is the exception: only with c_prev by value does the compiler fuse the same product of
// c = f c_prev + i g into the multiply-add as it did in the written-out per-step kernel (the other choice rounds differently).
#pragma once
#include "mtl_common.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// dropout convention of every recurrent kernel: u8 keep flags (NULL = no dropout), kept values scaled by mscale.  Serves the dropped
// copy of an output and the masked gradient from above alike.
__device__ __forceinline__ float dropped(float v, const uint8_t* mask, long e, float mscale) { return mask ? (mask[e] ? v * mscale : 0.f) : v; }
// ... of element e of a tensor, which is read only where it is kept
__device__ __forceinline__ float dropped(const float* v, const uint8_t* mask, long e, float mscale) {
    return mask ? (mask[e] ? v[e] * mscale : 0.f) : v[e];
}

// ------------------------------------------------------------------------------------------------------------------------- LSTM
// torch gate order i | f | g | o, pre = the four pre-activations (gx + gh):
//   i, f, o = sigmoid, g = tanh;  c = f c_prev + i g;  h = o tanh(c)
struct LstmAct {
    float i, f, g, o, c, h;
};
__device__ __forceinline__ LstmAct lstm_cell_act(const float (&pre)[4], float c_prev) {
    LstmAct a;
    a.i = sigmoidf_(pre[0]), a.f = sigmoidf_(pre[1]), a.g = tanhf(pre[2]), a.o = sigmoidf_(pre[3]);
    a.c = a.f * c_prev + a.i * a.g;
    a.h = a.o * tanhf(a.c);
    return a;
}
// dh = dh_up [* mask * mscale] + dh_rec;  dc = dc_next + dh o (1 - tanh(c)^2);  di = dc g, df = dc c_prev, dg = dc i, do = dh tanh(c),
// each through its sigmoid' / tanh' (-> the gradients of the pre-activations);  dc_prev = dc f.  dc_next: element e of a tensor that
// may be NULL (then 0: the last step);  c_prev: address of the value
struct LstmGrad {
    float di, df, dg, do_, dc_prev;
};
__device__ __forceinline__ LstmGrad lstm_cell_grad(float dh, const float* dc_next, long e, float i, float f, float g, float o, float c,
                                                   const float* c_prev) {
    const float tc = tanhf(c);
    const float dc = (dc_next ? dc_next[e] : 0.f) + dh * o * (1.f - tc * tc);
    LstmGrad d;
    d.di = dc * g * i * (1.f - i);
    d.df = dc * *c_prev * f * (1.f - f);
    d.dg = dc * i * (1.f - g * g);
    d.do_ = dh * tc * o * (1.f - o);
    d.dc_prev = dc * f;
    return d;
}

// -------------------------------------------------------------------------------------------------------------------------- GRU
// torch gate order r | z | n, gx = x W_ih^T + b_ih, gh = h W_hh^T + b_hh:
//   r = sigmoid(gx_r + gh_r)   z = sigmoid(gx_z + gh_z)   q = gh_n   n = tanh(gx_n + r q)   h' = (1 - z) n + z h
// gx, gh: the gate values at e, e + stride, e + 2 stride (a row of a (B, 3H) tensor: stride = H);  h_prev: address of the value
struct GruAct {
    float r, z, n, q, h;
};
__device__ __forceinline__ GruAct gru_cell_act(const float* gx, const float* gh, long e, int stride, const float* h_prev) {
    const float r = sigmoidf_(gx[e] + gh[e]), z = sigmoidf_(gx[e + stride] + gh[e + stride]), q = gh[e + 2 * stride];
    const float n = tanhf(gx[e + 2 * stride] + r * q);
    return GruAct{r, z, n, q, (1.f - z) * n + z * *h_prev};
}
// dh = masked gradient from above + recurrent gradient + direct carry:
//   dn = dh (1 - z)   dz = dh (h - n)   carry = dh z   da_n = dn (1 - n^2)   dq = da_n r   da_r = da_n q r (1 - r)   da_z = dz z (1 - z)
struct GruGrad {
    float da_r, da_z, da_n, dq, carry;
};
__device__ __forceinline__ GruGrad gru_cell_grad(float dh, float r, float z, float n, float q, float hprev) {
    const float dn = dh * (1.f - z), dz = dh * (hprev - n);
    GruGrad g;
    g.da_n = dn * (1.f - n * n);
    g.dq = g.da_n * r;
    g.da_r = g.da_n * q * r * (1.f - r);
    g.da_z = dz * z * (1.f - z);
    g.carry = dh * z;
    return g;
}

}  // namespace
