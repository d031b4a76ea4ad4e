// mfma_probe.hip -- prints where v_mfma_f32_32x32x2_f32 puts D[i][j] (lane, register), measured, and the
// largest difference between the MFMA dot products and the lane-ordered fp32 sums the distance kernels use,
// as a fraction of the margin the heuristic's prefilter allows for it (csrc/dk_heuristic.h: E, Esq).
//   mfma_probe                 uniform unit rows, K = 768, generated here
//   mfma_probe rows.f32 K      a row family: raw float32 rows of K floats (K % 8 == 0), 64 per group -- the first 32
//                              of a group against its last 32 (python tests/gram_prefilter.py <case id> rows.f32 writes one)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
typedef float floatx16 __attribute__((ext_vector_type(16)));
__global__ void probe(const float *A /*32 x K row-major*/, const float *B /*32 x K row-major*/, int K, float *out /*64 x 16*/)
{
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    floatx16 acc = {0};
    for (int k0 = 0; k0 < K; k0 += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[r * K + k0 + h], B[r * K + k0 + h], acc, 0, 0, 0);
    for (int v = 0; v < 16; ++v) out[lane * 16 + v] = acc[v];
}
// D[i][j] of a probe result under the layout j = lane % 32, i = 8 (v / 4) + 4 (lane / 32) + v % 4
static float at(const std::vector<float> &out, int i, int j)
{
    const int h = (i >> 2) & 1, v = 4 * (i >> 3) + (i & 3);
    return out[(j + 32 * h) * 16 + v];
}
int main(int argc, char **argv)
{
    int K = 768;
    std::vector<float> rows;
    if (argc >= 3) {
        K = atoi(argv[2]);
        FILE *f = fopen(argv[1], "rb");
        if (!f || K <= 0 || K % 8) { fprintf(stderr, "usage: mfma_probe [rows.f32 K]   (K %% 8 == 0)\n"); return 2; }
        float buf[4096];
        size_t got;
        while ((got = fread(buf, 4, 4096, f)) > 0) rows.insert(rows.end(), buf, buf + got);
        fclose(f);
    } else {
        rows.resize(64 * K);
        srand(7);
        for (auto &x : rows) x = rand() / (float)RAND_MAX;
        for (int i = 0; i < 64; ++i) { // unit rows
            double n = 0;
            for (int k = 0; k < K; ++k) n += (double)rows[i * K + k] * rows[i * K + k];
            for (int k = 0; k < K; ++k) rows[i * K + k] /= (float)sqrt(n);
        }
    }
    const int groups = (int)(rows.size() / (size_t)(64 * K));
    if (groups < 1) { fprintf(stderr, "need at least 64 rows of %d floats\n", K); return 2; }
    float *dR, *dO;
    hipMalloc(&dR, (size_t)64 * K * 4); hipMalloc(&dO, 64 * 16 * 4);
    const double u = ldexp(1.0, -24), E = (1.125 * K + 32) * u, Esq = (2.25 * K + 32) * u * 1.01;
    double worst_guess = 0, worst_dot = 0, worst_dot_frac = 0, worst_sq = 0, worst_sq_frac = 0;
    std::vector<float> ab(64 * 16), aa(64 * 16), bb(64 * 16);
    for (int g = 0; g < groups; ++g) {
        const float *A = rows.data() + (size_t)g * 64 * K, *B = A + 32 * K;
        hipMemcpy(dR, A, (size_t)64 * K * 4, hipMemcpyHostToDevice);
        const float *dA = dR, *dB = dR + 32 * K;
        hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, K, dO); hipMemcpy(ab.data(), dO, ab.size() * 4, hipMemcpyDeviceToHost);
        hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dA, K, dO); hipMemcpy(aa.data(), dO, aa.size() * 4, hipMemcpyDeviceToHost);
        hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dB, dB, K, dO); hipMemcpy(bb.data(), dO, bb.size() * 4, hipMemcpyDeviceToHost);
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                // guess: D[i][j] with j = lane % 32, i = 8 * (v / 4) + 4 * (lane / 32) + v % 4
                const float m = at(ab, i, j);
                double ref = 0, na = 0, nb = 0;
                for (int k = 0; k < K; ++k) { ref += (double)A[i * K + k] * (double)B[j * K + k]; na += (double)A[i * K + k] * A[i * K + k]; nb += (double)B[j * K + k] * B[j * K + k]; }
                const double len = sqrt(na) * sqrt(nb);
                if (std::isfinite(ref) && std::isfinite(len) && len > 0) worst_guess = fmax(worst_guess, fabs(ref - m) / len);
                // the kernels' order: 8 partial sums, element k -> partial k % 8, mul then add, tree (p0+p4 + p2+p6) + (p1+p5 + p3+p7)
                float p[8] = {0}, q[8] = {0};
                for (int k = 0; k < K; ++k) {
                    float pr = A[i * K + k] * B[j * K + k]; p[k % 8] = p[k % 8] + pr;
                    float d = A[i * K + k] - B[j * K + k]; q[k % 8] = fmaf(d, d, q[k % 8]); // sq_euclid: fused, tree (q0+q4 + q1+q5) + (q2+q6 + q3+q7)
                }
                const float s = ((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7]));
                const float sq = ((q[0] + q[4]) + (q[1] + q[5])) + ((q[2] + q[6]) + (q[3] + q[7]));
                const double dd = fabs((double)s - m);
                if (std::isfinite(dd) && len > 0) { worst_dot = fmax(worst_dot, dd); worst_dot_frac = fmax(worst_dot_frac, dd / (E * fmax(len, 1e-300))); }
                const float nn = at(aa, i, i) + at(bb, j, j), tile_sq = nn - 2.0f * m;
                const double ds = fabs((double)tile_sq - sq);
                if (std::isfinite(ds) && nn > 0) { worst_sq = fmax(worst_sq, ds); worst_sq_frac = fmax(worst_sq_frac, ds / (Esq * nn)); }
            }
    }
    printf("layout guess j=lane%%32, i=8*(v/4)+4*(lane/32)+v%%4: max |D - float64 dot| / (|a||b|) = %.3e (%s)\n", worst_guess, worst_guess < 1e-4 ? "CONFIRMED" : "WRONG");
    printf("K = %d, %d pairs (%s): max |MFMA - lane-ordered fp32| = %.3e = %.4f of E |a||b| (E = %.3e); sq_euclid off the tiles: max |n_i + n_j - 2 D - lane-ordered| = %.3e = %.4f of Esq (n_i + n_j)\n",
           K, groups * 1024, argc >= 3 ? argv[1] : "uniform unit rows", worst_dot, worst_dot_frac, E, worst_sq, worst_sq_frac);
    return worst_guess < 1e-4 ? 0 : 1;
}
