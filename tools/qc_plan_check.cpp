// qc_plan_check.cpp -- the pure functions the QC report adds to csrc/sdt_read_plan.h, on the CPU under sanitizers (tests/test_read_qc_host.py):
// every refusal of check_qc_params with the values next to it and the order of the checks, the layout of the report against the table
// of include/sdt_gpu.h, and the grid.  Prints the kernel's tile rows and wavefronts, which the binding and the tests restate.
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace sdt;

#define CHECK(cond)                                                          \
	do {                                                                     \
		if (!(cond)) {                                                       \
			std::fprintf(stderr, "qc_plan_check: %s (line %d)\n", #cond, __LINE__); \
			std::exit(1);                                                    \
		}                                                                    \
	} while (0)

int main()
{
	const QcParams good = {150, 33, 0, 0, 0};
	CHECK(check_qc_params(good) == QC_OK);
	// cycles
	for (uint32_t c : {0u, 4097u, 0xFFFFFFFFu}) { QcParams p = good; p.cycles = c; CHECK(check_qc_params(p) == QC_CYCLES); }
	for (uint32_t c : {1u, 2u, 4095u, 4096u}) { QcParams p = good; p.cycles = c; CHECK(check_qc_params(p) == QC_OK); }
	// phred_offset: exactly 0, 33, 64
	for (uint32_t v = 0; v < 300; v++) {
		QcParams p = good;
		p.phred_offset = v;
		CHECK(check_qc_params(p) == ((v == 0 || v == 33 || v == 64) ? QC_OK : QC_PHRED_OFFSET));
	}
	// flags: SDT_QC_FROM_END and nothing else
	for (int b = 0; b < 32; b++) {
		QcParams p = good;
		p.flags = 1u << b;
		CHECK(check_qc_params(p) == (b == 0 ? QC_OK : QC_FLAGS));
		p.flags |= 1u;
		CHECK(check_qc_params(p) == (b == 0 ? QC_OK : QC_FLAGS));
	}
	// class_sel: a byte
	for (uint32_t v : {0u, 1u, 2u, 255u}) { QcParams p = good; p.class_sel = v; CHECK(check_qc_params(p) == QC_OK); }
	for (uint32_t v : {256u, 257u, 0xFFFFFFFFu}) { QcParams p = good; p.class_sel = v; CHECK(check_qc_params(p) == QC_CLASS_SEL); }
	// reserved
	for (uint32_t v : {1u, 0x80000000u}) { QcParams p = good; p.reserved = v; CHECK(check_qc_params(p) == QC_RESERVED); }
	// the first field that is refused, in the order of the rule
	{
		QcParams p = {0, 7, 2, 256, 1};
		CHECK(check_qc_params(p) == QC_CYCLES);
		p.cycles = 1;
		CHECK(check_qc_params(p) == QC_PHRED_OFFSET);
		p.phred_offset = 64;
		CHECK(check_qc_params(p) == QC_FLAGS);
		p.flags = 1;
		CHECK(check_qc_params(p) == QC_CLASS_SEL);
		p.class_sel = 255;
		CHECK(check_qc_params(p) == QC_RESERVED);
		p.reserved = 0;
		CHECK(check_qc_params(p) == QC_OK);
	}
	// the layout: totals 8, base 4 R, qual 94 R, len R, gc 101, meanq 94, in this order and without gaps: 203 + 99 R
	for (uint32_t C = 1; C <= QC_MAX_CYCLES; C++) {
		const QcLayout l = qc_layout(C);
		const uint64_t R = (uint64_t)C + 1;
		CHECK(l.rows == R && l.totals == 0 && l.base == 8 && l.qual == l.base + 4 * R && l.len == l.qual + 94 * R && l.gc == l.len + R);
		CHECK(l.meanq == l.gc + 101 && l.words == l.meanq + 94 && l.words == 203 + 99 * R);
		CHECK(qc_report_words(C) == l.words);
	}
	CHECK(qc_report_words(0) == 0 && qc_report_words(QC_MAX_CYCLES + 1) == 0 && qc_report_words(0xFFFFFFFFu) == 0);
	CHECK(qc_report_words(150) == 15152 && qc_report_words(4096) == 405806);
	// the grid: one workgroup per QC_WAVES reads, two per CU at most, the hook in the place of that cap, never none
	CHECK(qc_blocks(0, 256, 0) == 1 && qc_blocks(1, 256, 0) == 1 && qc_blocks(QC_WAVES, 256, 0) == 1 && qc_blocks(QC_WAVES + 1, 256, 0) == 2);
	CHECK(qc_blocks(1ULL << 40, 256, 0) == 512 && qc_blocks(1ULL << 40, 304, 0) == 608 && qc_blocks(1ULL << 40, 0, 0) == 2);
	CHECK(qc_blocks(1ULL << 40, 256, 3) == 3 && qc_blocks(20000, 256, 1) == 1 && qc_blocks(5, 256, 3) == 1);
	CHECK(qc_blocks(~0ULL, 256, 0) == 512);
	// the LDS of a workgroup: the tile with its odd row stride, len, gc, meanq, row C in 64 bits and one word; two of them per CU
	const uint64_t lds = (uint64_t)QC_TILE * 99 * 4 + (QC_MAX_CYCLES + 1) * 4 + QC_GC_BINS * 4 + QC_QUALS * 4 + 98 * 8 + 8;
	CHECK(2 * lds <= 160 * 1024 && QC_TILE >= 151);
	std::printf("qc_plan_check: ok tile %d waves %d\n", QC_TILE, QC_WAVES);
	return 0;
}
