// mul_rate_probe.hip -- what a 32-bit multiply costs next to a 24-bit one and a plain vector instruction on this GPU.
//   hipcc -O3 --offload-arch=gfx950 -o mul_rate_probe mul_rate_probe.hip && ./mul_rate_probe
// Every lane runs ITERS rounds of 8 independent chains of ONE instruction (v_mul_lo_u32, v_mul_u32_u24, v_xor_b32); 8 waves per SIMD
// keep the issue port busy, so the time per instruction is its issue cost.  Prints ns per wave-instruction and SIMD and the ratios.
// (profiles/l1_walk/README.md: whether the m-mer hash of the level-1 scatter's walk should split its multiply, sdt_sk_walk.h.)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int ITERS = 4096, CHAINS = 8;

template <int OP> __global__ __launch_bounds__(512) void k_chain(uint32_t *out, uint32_t c)
{
	uint32_t x[CHAINS];
	for (int i = 0; i < CHAINS; i++)
		x[i] = threadIdx.x * 2654435761u + (uint32_t)i;
	for (int it = 0; it < ITERS; it++) {
#pragma unroll
		for (int i = 0; i < CHAINS; i++) {
			if (OP == 0) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(x[i]) : "v"(c));
			if (OP == 1) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(x[i]) : "v"(c));
			if (OP == 2) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(x[i]) : "v"(c));
		}
	}
	uint32_t s = 0;
	for (int i = 0; i < CHAINS; i++)
		s ^= x[i];
	if (s == 0x12345u)                           // (keeps the chains alive; practically never true)
		out[blockIdx.x] = s;
}

template <int OP> static double run(uint32_t *d_out, int grid)
{
	hipEvent_t e0, e1;
	HIPCHK(hipEventCreate(&e0));
	HIPCHK(hipEventCreate(&e1));
	hipLaunchKernelGGL(k_chain<OP>, dim3(grid), dim3(512), 0, 0, d_out, 0x9E3779B1u);      // warm-up
	HIPCHK(hipDeviceSynchronize());
	float best = 1e30f;
	for (int rep = 0; rep < 5; rep++) {
		HIPCHK(hipEventRecord(e0));
		hipLaunchKernelGGL(k_chain<OP>, dim3(grid), dim3(512), 0, 0, d_out, 0x9E3779B1u);
		HIPCHK(hipEventRecord(e1));
		HIPCHK(hipEventSynchronize(e1));
		float ms;
		HIPCHK(hipEventElapsedTime(&ms, e0, e1));
		best = ms < best ? ms : best;
	}
	return best;
}

int main()
{
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, 0));
	const int cus = prop.multiProcessorCount, grid = cus * 4;        // 4 workgroups of 8 waves per CU: 8 waves per SIMD
	uint32_t *d_out;
	HIPCHK(hipMalloc(&d_out, (size_t)grid * 4));
	const double ms[3] = {run<0>(d_out, grid), run<1>(d_out, grid), run<2>(d_out, grid)};
	const char *name[3] = {"v_mul_lo_u32", "v_mul_u32_u24", "v_xor_b32"};
	const double per_simd = 8.0 * ITERS * CHAINS;                      // wave-instructions per SIMD
	for (int i = 0; i < 3; i++)
		printf("%-14s %8.3f ms  %6.2f ns per wave-instruction and SIMD  %5.2f x v_xor_b32\n", name[i], ms[i], ms[i] * 1e6 / per_simd, ms[i] / ms[2]);
	printf("mul_rate_probe: %s, %d CUs, clock %d MHz\n", prop.name, cus, prop.clockRate / 1000);
	HIPCHK(hipFree(d_out));
	return 0;
}
