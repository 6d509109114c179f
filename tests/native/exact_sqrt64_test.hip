// Is the binary64 square root the gradient rule of vgx_raster_painted calls on the device the IEEE one? vgx_raster_sqrt of
// csrc/vgx_raster.h -- the very function the lane code calls -- runs on the device over about 2^26 inputs and is compared bit for bit
// with the same function on the host (x86-64: sqrtsd, correctly rounded):
//   squares   ox*ox + oy*oy of two binary32 values widened, as the rule forms them, from the ranges a frame produces: distances of a
//             fraction of a pixel up to 2^20 pixels, and the 1e5-sized extents of a linear gradient
//   binades   random significands in every binade of binary64, the subnormals included
//   perfect   n*n for integers and half-integers n, and the two neighbours of each: where a wrong last step shows first
//   special   +-0, infinity, NaN, a negative number (both sides must give a NaN there; its bits play no part in the rule)
// Prints one line per class, "<name> mismatches=<n> of <total>", and "mismatches=<n> of <N>" for all of them. Built by
// __graft_entry__.build() and run by tests/test_gpu_exact_sqrt64.py; exit code 1 when any input differs.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "../../vg-renderer_amd/csrc/vgx_raster.h"

__global__ void k_sqrt(const double* x, double* r, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) { r[i] = vgx_raster_sqrt(x[i]); }
}

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t next64() // splitmix64
{
	uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
static double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t to_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
// a binary32 value with a random significand and an exponent in [e0, e1]
static float rand_float(int e0, int e1)
{
	const uint64_t r = next64();
	const float m = 1.0f + (float)(r & 0x7FFFFFu) / 8388608.0f; // exact: 23 bits
	return ldexpf(m, e0 + (int)((r >> 32) % (uint64_t)(e1 - e0 + 1)));
}

static const uint32_t CHUNK = 1u << 22;

struct Checker
{
	double *dx, *dr;
	std::vector<double> x, r;
	unsigned long long total, bad;
	Checker() : x(), r(CHUNK), total(0), bad(0)
	{
		if (hipMalloc(&dx, CHUNK * sizeof(double)) != hipSuccess || hipMalloc(&dr, CHUNK * sizeof(double)) != hipSuccess) { printf("hipMalloc failed\n"); exit(2); }
		x.reserve(CHUNK);
	}
	void flush(unsigned long long* classBad)
	{
		const uint32_t n = (uint32_t)x.size();
		if (!n) { return; }
		if (hipMemcpy(dx, x.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { printf("upload failed\n"); exit(2); }
		hipLaunchKernelGGL(k_sqrt, dim3((n + 255u) / 256u), dim3(256), 0, 0, dx, dr, n);
		if (hipMemcpy(r.data(), dr, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel or download failed\n"); exit(2); }
		for (uint32_t i = 0; i < n; ++i) {
			const double want = vgx_raster_sqrt(x[i]);
			if (to_bits(want) != to_bits(r[i]) && !(want != want && r[i] != r[i])) {
				if (bad + *classBad < 8) { printf("  sqrt(%a): device %a, host %a\n", x[i], r[i], want); }
				++*classBad;
			}
		}
		total += n;
		x.clear();
	}
	void add(double v, unsigned long long* classBad)
	{
		x.push_back(v);
		if (x.size() == CHUNK) { flush(classBad); }
	}
};

int main()
{
	Checker c;
	unsigned long long b = 0, before;
	// squares: 2^25
	before = c.total;
	for (uint32_t i = 0; i < (1u << 25); ++i) {
		double ox, oy;
		switch (i & 3u) {
		case 0: ox = (double)rand_float(-8, 12); oy = (double)rand_float(-8, 12); break;   // pixels
		case 1: ox = (double)rand_float(-20, 20); oy = (double)rand_float(-20, 20); break; // any two magnitudes
		case 2: ox = (double)rand_float(0, 11); oy = 0.0; break;                           // one axis inside the rectangle: sqrt of a square
		default: ox = (double)rand_float(10, 17); oy = (double)rand_float(-4, 17); break;  // the 1e5-sized extents of a linear gradient
		}
		c.add(ox * ox + oy * oy, &b);
	}
	c.flush(&b);
	printf("squares mismatches=%llu of %llu\n", b, c.total - before);
	c.bad += b; b = 0;
	// binades: 2047 x 2^13 (the exponents 0 .. 2046: subnormals to the largest binade)
	before = c.total;
	for (uint32_t k = 0; k < (1u << 13); ++k) {
		for (uint64_t e = 0; e < 2047u; ++e) { c.add(from_bits((e << 52) | (next64() >> 12)), &b); }
	}
	c.flush(&b);
	printf("binades mismatches=%llu of %llu\n", b, c.total - before);
	c.bad += b; b = 0;
	// perfect squares and their neighbours: 3 x 2^22 integers and half-integers below 2^26 (n * n is exact)
	before = c.total;
	for (uint32_t i = 0; i < (1u << 22); ++i) {
		const double n = (double)(next64() >> (38 + (i & 15u))) * ((i & 16u) ? 0.5 : 1.0) + 1.0;
		const double s = n * n;
		c.add(s, &b); c.add(nextafter(s, 0.0), &b); c.add(nextafter(s, INFINITY), &b);
	}
	c.flush(&b);
	printf("perfect mismatches=%llu of %llu\n", b, c.total - before);
	c.bad += b; b = 0;
	before = c.total;
	const double special[] = { 0.0, -0.0, INFINITY, NAN, -1.0, from_bits(1), from_bits(0x7FEFFFFFFFFFFFFFull), 1.0, 2.0, 4.0 };
	for (double v : special) { c.add(v, &b); }
	c.flush(&b);
	printf("special mismatches=%llu of %llu\n", b, c.total - before);
	c.bad += b;
	printf("mismatches=%llu of %llu\n", c.bad, c.total);
	(void)hipFree(c.dx); (void)hipFree(c.dr);
	return c.bad ? 1 : 0;
}
