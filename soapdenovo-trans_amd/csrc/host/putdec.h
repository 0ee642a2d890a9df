/* putdec.h -- the one writer of unsigned decimals of the host tools' text files (8 M reads are 180 MB of digits: formatted by hand) */
#ifndef SDT_PUTDEC_H
#define SDT_PUTDEC_H
#include <stdint.h>

/* v in decimal and then sep; returns the end of what it wrote (at most 21 bytes, 11 for a value of 32 bits) */
static inline char *sdt_put_dec(char *p, uint64_t v, char sep)
{
	char t[20];
	int n = 0;
	for (; v > UINT32_MAX; v /= 10) t[n++] = (char)('0' + v % 10);
	uint32_t w = (uint32_t)v;                                                /* (the usual field: 32-bit arithmetic) */
	do { t[n++] = (char)('0' + w % 10); w /= 10; } while (w);
	while (n) *p++ = t[--n];
	*p++ = sep;
	return p;
}

#endif
