// Probe: absolute error of sin^2 evaluated three ways on gfx950, against f64.
//   (a) period-pi Cody-Waite + degree-5 polynomial (what conv_f16x3.hip uses), (b) 0.5 - 0.5 * v_cos_f32(t / pi turns), (c) v_sin_f32 squared
// Three sweeps: |t| <= 40 (the snake arguments of O(1) alpha and activations); t = alpha v for v in [-4, 4] per alpha of a grid, the
// error divided by alpha (what the snake v + sin^2(alpha v) / alpha makes of it); and bands of large |t| up to 9000 rad, across and
// beyond +-256 turns of the trig instructions' argument (|t| = 804 for the cosine of the doubled angle, 1608 for the sine).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
__device__ float sin_sq_poly(float t) {  // the form used by conv_f16x3.hip
    const float n = rintf(t * 0.318309886183790672f);
    float r = fmaf(n, -3.14159274101257324f, t);
    r = fmaf(n, 8.74227765734758578e-08f, r);
    const float z = r * r;
    float p = fmaf(z, -3.6197402550897095e-06f, 1.3928599946666651e-04f);
    p = fmaf(z, p, -3.1722760759294033e-03f);
    p = fmaf(z, p, 4.4443082064390182e-02f);
    p = fmaf(z, p, -3.3333304524421692e-01f);
    p = fmaf(z, p, 1.0f);
    return z * p;
}
__global__ void k(const float* t, float* o, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = t[i];
    o[i] = sin_sq_poly(x);
    o[n + i] = fmaf(-0.5f, __builtin_amdgcn_cosf(x * 0.318309886183790672f), 0.5f);  // cos(2x) = cos(2 pi * x/pi)
    const float sv = __builtin_amdgcn_sinf(x * 0.159154943091895336f);
    o[2 * n + i] = sv * sv;
}
static const char* names[3] = {"poly", "0.5-0.5*v_cos(x/pi)", "v_sin(x/2pi)^2"};
// the three forms on the arguments h (float32), error against sin^2 of the same float32 argument in f64, times `mul`
static void sweep(const char* what, const std::vector<float>& h, double mul) {
    const int n = (int)h.size();
    float *d, *o;
    hipMalloc(&d, (size_t)n * 4); hipMalloc(&o, (size_t)3 * n * 4);
    hipMemcpy(d, h.data(), (size_t)n * 4, hipMemcpyHostToDevice);
    k<<<(n + 255) / 256, 256>>>(d, o, n);
    std::vector<float> r((size_t)3 * n);
    hipMemcpy(r.data(), o, (size_t)3 * n * 4, hipMemcpyDeviceToHost);
    hipFree(d); hipFree(o);
    for (int m = 0; m < 3; ++m) {
        double worst = 0, sum = 0, sq = 0;
        for (int i = 0; i < n; ++i) {
            const double ref = std::sin((double)h[i]);
            const double e = std::fabs((double)r[(size_t)m * n + i] - ref * ref) * mul;
            worst = e > worst ? e : worst; sum += e; sq += e * e;
        }
        printf("%-28s %-22s max abs err %.3e  mean %.3e  rms %.3e\n", what, names[m], worst, sum / n, std::sqrt(sq / n));
    }
}
int main() {
    const int n = 1 << 22;
    std::vector<float> h(n);
    for (int i = 0; i < n; ++i) h[i] = -40.f + 80.f * (float)i / n;  // |alpha * y| range of the snake arguments
    sweep("|t| <= 40", h, 1.0);
    // the snake's own error: sin^2(alpha v) / alpha for v in [-4, 4], the product alpha v rounded to float32 as the kernels round it
    const float alphas[7] = {0.01f, 0.02f, 0.05f, 0.2f, 1.f, 5.f, 20.f};
    for (int a = 0; a < 7; ++a) {
        for (int i = 0; i < n; ++i) h[i] = alphas[a] * (-4.f + 8.f * (float)i / n);
        char what[64];
        snprintf(what, sizeof what, "err / alpha, alpha = %g", alphas[a]);
        sweep(what, h, 1.0 / alphas[a]);
    }
    // large arguments: inside +-256 turns of the cosine's argument, between the cosine's and the sine's limit, and far beyond both
    const float bands[4][2] = {{40.f, 800.f}, {810.f, 1600.f}, {1620.f, 9000.f}, {9000.f, 100000.f}};
    for (int b = 0; b < 4; ++b) {
        for (int i = 0; i < n; ++i) {
            const float m = bands[b][0] + (bands[b][1] - bands[b][0]) * (float)(i >> 1) / (n >> 1);
            h[i] = (i & 1) ? -m : m;
        }
        char what[64];
        snprintf(what, sizeof what, "%g <= |t| <= %g", bands[b][0], bands[b][1]);
        sweep(what, h, 1.0);
    }
    return 0;
}
