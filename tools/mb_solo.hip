// Microbenchmark (diagnostic, not product): the LATENCY of one Newton-matrix
// LDL^T (Go2: 24 x 24) for a lone straggler env -- what a wavefront whose other env rows have
// finished could gain by spreading the straggler's factor over the idle rows.  One wavefront in
// the whole grid (nothing else on the GPU), clock64() around REPS factorisations:
//   A  (product) ldl_rows<24> of osc_ipm.hpp: one 16-lane DPP row per env, lane l holds columns
//      l and l+16 (four envs per wave; the other three rows are the finished env rows, they run
//      the same instructions in lockstep);
//   B  the straggler over 32 lanes: two 16-lane rows, row r the entries i = r (mod 2) of columns
//      l, l+16 -- a pivot column's entries are DPP-broadcast inside each row, half the trailing
//      FMAs per lane; the pivot and the multipliers -L[j][k] cross from the owner row once per
//      step (__shfl);
//   C  the straggler over all 64 lanes: four rows, row r the entries i = r (mod 4): a quarter of
//      the trailing FMAs per lane, the same per-step crossings.
// Plus the product's two triangular solves (ldl_solve_rows, one pass's) for the share they take.
// Each factor is checked against a host LDL^T.  Prints one JSON line.
//   hipcc -std=c++17 -O3 --offload-arch=gfx950 -I operational-space-control_amd/csrc \
//         -I include tools/mb_solo.hip -o /tmp/mb_solo
#include "osc_ipm.hpp"
#include <cmath>
#include <cstdio>
#include <vector>

using namespace osc;

constexpr int N = 24, REPS = 64;

__device__ __forceinline__ double kval(int i, int j) {   // SPD, diagonally dominant
  const double off = 1.0 / (1.0 + ((i * 7 + j * 7 + (i == j ? 0 : i * j)) % 11));
  return i == j ? 2.0 * N : off;
}

// A: the product's factor (and one pass's two triangular solves)
__global__ __launch_bounds__(64, 1) void k_a(double* out, unsigned long long* clk) {
  __shared__ double sdinv[4][2 * kRow];
  const int lane = threadIdx.x, grp = lane / kRow, l = lane % kRow;
  const int j1 = l + kRow < N ? l + kRow : N - 1;
  double k0[N], k1[N];
  for (int i = 0; i < N; ++i) {
    k0[i] = kval(i, l);
    k1[i] = kval(i, j1);
  }
  double acc = 0.0;
  unsigned long long tf = 0, ts = 0;
  for (int rep = 0; rep < REPS; ++rep) {
    double c0[N], c1[N];
    for (int i = 0; i < N; ++i) {
      c0[i] = k0[i] + 1e-3 * rep;
      c1[i] = k1[i] + 1e-3 * rep;
    }
    double d0, d1;
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t0 = clock64();
    ldl_rows<N>(c0, c1, sdinv[grp], l, d0, d1, 1e-13 * k0[l], 1e-13 * k1[j1], 0.0);
    const unsigned long long t1 = clock64();
    double a0 = 1.0 + l, a1 = 2.0 + l;
    ldl_solve_rows<N>(c0, c1, d0, d1, a0, a1, l);
    const unsigned long long t2 = clock64();
    tf += t1 - t0;
    ts += t2 - t1;
    acc += a0 + a1;
    if (rep == REPS - 1 && grp == 0)
      for (int i = 0; i < N; ++i) {
        out[i * N + l] = c0[i];
        if (l + kRow < N) out[i * N + l + kRow] = c1[i];
      }
  }
  if (acc == 12345.678) out[0] = acc;   // keep the loop
  if (lane == 0) {
    clk[0] = tf;
    clk[1] = ts;
  }
}

// B / C: one env over R rows (R = 2 or 4), row r holding the entries i = r (mod R)
template <int R>
__global__ __launch_bounds__(64, 1) void k_split(double* out, unsigned long long* clk) {
  constexpr int MR = N / R;
  const int lane = threadIdx.x, r = (lane >> 4) % R, l = lane & 15;
  const int j1 = l + kRow < N ? l + kRow : N - 1;
  double k0[MR], k1[MR];
  for (int m = 0; m < MR; ++m) {
    k0[m] = kval(R * m + r, l);
    k1[m] = kval(R * m + r, j1);
  }
  double acc = 0.0;
  unsigned long long tf = 0;
  for (int rep = 0; rep < REPS; ++rep) {
    double e0[MR], e1[MR];
    for (int m = 0; m < MR; ++m) {
      e0[m] = k0[m] + 1e-3 * rep;
      e1[m] = k1[m] + 1e-3 * rep;
    }
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t0 = clock64();
    static_for<0, N>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      constexpr int ro = k % R, mk = k / R, s = k / kRow, kl = k % kRow;
      const int src = (lane & ~(R * kRow - 1)) + ro * kRow + l;   // same lane of the owner row
      const double own = (s == 0) ? e0[mk] : e1[mk];
      const double dk = __shfl(bcast_guarded<kl>(own), src);      // pivot D_k
      const double inv = recip1(dk);
      double t0v = __shfl(-e0[mk] * inv, src), t1v = __shfl(-e1[mk] * inv, src);
      t0v = keep_lanes<rows_mask(lanes_from(k + 1, 15))>(t0v);   // slot-0 columns still to go
      constexpr unsigned kT1 = (k < kRow) ? lanes_from(0, N - 1 - kRow)
                                          : lanes_from(k + 1 - kRow, N - 1 - kRow);
      t1v = keep_lanes<rows_mask(kT1)>(t1v);
      // at m == mk only the rows r > ro hold an entry (R mk + r) below the pivot
      const double tm0 = r > ro ? t0v : 0.0, tm1 = r > ro ? t1v : 0.0;
      static_for<mk, MR>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const double u0 = (m == mk) ? tm0 : t0v;
        const double u1 = (m == mk) ? tm1 : t1v;
        if constexpr (s == 0) {
          fmac_bcast<kl>(e1[m], e0[m], u1);
          fmac_bcast_self<kl>(e0[m], u0);
        } else {
          fmac_bcast_self<kl>(e1[m], u1);
        }
      });
    });
    const unsigned long long t1 = clock64();
    tf += t1 - t0;
    acc += e0[0] + e1[0];
    if (rep == REPS - 1 && lane < R * kRow)
      for (int m = 0; m < MR; ++m) {
        out[(R * m + r) * N + l] = e0[m];
        if (l + kRow < N) out[(R * m + r) * N + l + kRow] = e1[m];
      }
  }
  if (acc == 12345.678) out[0] = acc;
  if (lane == 0) clk[0] = tf;
}

// entries below the diagonal after the right-looking elimination: L[i][j] D_j (split kernels);
// the product's are pre-scaled by -1/D_i (ldl_rows' contract)
static double check(const std::vector<double>& F, bool prescaled) {
  std::vector<double> A(N * N), L(N * N, 0.0), D(N);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      const double off = 1.0 / (1.0 + ((i * 7 + j * 7 + (i == j ? 0 : i * j)) % 11));
      A[i * N + j] = (i == j ? 2.0 * N : off) + 1e-3 * (REPS - 1);
    }
  for (int k = 0; k < N; ++k) {
    D[k] = A[k * N + k];
    for (int i = k + 1; i < N; ++i) L[i * N + k] = A[i * N + k] / D[k];
    for (int i = k + 1; i < N; ++i)
      for (int j = k + 1; j < N; ++j) A[i * N + j] -= L[i * N + k] * D[k] * L[j * N + k];
  }
  double e = 0.0;
  for (int j = 0; j < N; ++j)
    for (int i = j + 1; i < N; ++i) {
      const double want = prescaled ? -L[i * N + j] * D[j] / D[i] : L[i * N + j] * D[j];
      e = fmax(e, fabs(F[i * N + j] - want));
    }
  return e;
}

int main() {
  double* dout;
  unsigned long long* dclk;
  (void)hipMalloc(&dout, N * N * sizeof(double));
  (void)hipMalloc(&dclk, 4 * sizeof(unsigned long long));
  std::vector<double> F(N * N);
  unsigned long long clk[4];
  double cyc[3], err[3], solve = 0.0;
  for (int v = 0; v < 3; ++v) {
    unsigned long long best_f = ~0ull, best_s = ~0ull;
    for (int trial = 0; trial < 5; ++trial) {   // first launch warms the I-cache
      (void)hipMemset(dout, 0, N * N * sizeof(double));
      if (v == 0) hipLaunchKernelGGL(k_a, dim3(1), dim3(64), 0, 0, dout, dclk);
      if (v == 1) hipLaunchKernelGGL(k_split<2>, dim3(1), dim3(64), 0, 0, dout, dclk);
      if (v == 2) hipLaunchKernelGGL(k_split<4>, dim3(1), dim3(64), 0, 0, dout, dclk);
      (void)hipDeviceSynchronize();
      (void)hipMemcpy(clk, dclk, sizeof(clk), hipMemcpyDeviceToHost);
      best_f = clk[0] < best_f ? clk[0] : best_f;
      if (v == 0) best_s = clk[1] < best_s ? clk[1] : best_s;
    }
    (void)hipMemcpy(F.data(), dout, F.size() * sizeof(double), hipMemcpyDeviceToHost);
    cyc[v] = static_cast<double>(best_f) / REPS;
    err[v] = check(F, v == 0);
    if (v == 0) solve = static_cast<double>(best_s) / REPS;
  }
  printf("{\"n\": %d, \"clock\": \"clock64 per factorisation, one wavefront in the grid\", "
         "\"ldl_16lane_product\": %.0f, \"ldl_32lane\": %.0f, \"ldl_64lane\": %.0f, "
         "\"two_tri_solves_16lane_product\": %.0f, \"max_err\": [%.2e, %.2e, %.2e]}\n",
         N, cyc[0], cyc[1], cyc[2], solve, err[0], err[1], err[2]);
  return (err[0] < 1e-9 && err[1] < 1e-9 && err[2] < 1e-9) ? 0 : 1;
}
