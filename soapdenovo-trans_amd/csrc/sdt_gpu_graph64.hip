// sdt_gpu_graph64.hip -- the graph phases with 64-bit node indices (Ix64 of sdt_graph_kernels.cuh; part of libsdt_gpu.so).
// The entry points of sdt_gpu_graph.hip take this form past 2^32 - 16 nodes or when the caller asked for it
// (sdt_gpu_set_graph_index_bits); below that they run the Ix32 instantiations of the same templates, compiled over there.
#define SDT_GRAPH_WIDE_UNIT
#include "sdt_graph_phases.hpp"

template int sdti::tip_walks_labelled<Ix64>(sdt_ctx *, Ix64, int, int, uint64_t *);
template int sdti::minor_out_labelled<Ix64>(sdt_ctx *, Ix64, double, uint64_t *, uint64_t *);
template int sdti::minor_out_commit_begin<Ix64>(sdt_ctx *, Ix64, double, uint64_t, uint64_t *, uint64_t *, uint64_t *);
template int sdti::build_edges<Ix64>(sdt_ctx *, Ix64, uint64_t *, uint64_t *, uint64_t *);
template int sdti::layout_order<Ix64>(const GraphView &, const RpSet *, const unsigned long long *, int, const unsigned long long *, const uint32_t *, uint64_t, uint64_t *);
template int sdti::layout_number<Ix64>(const GraphView &, Ix64, const uint64_t *, const uint64_t *, uint64_t, uint64_t *, uint64_t *);
template int sdti::set_index<Ix64>(const GraphView &, Ix64, const uint64_t *, uint64_t);
template int sdti::host_index<Ix64, unsigned int>(const GraphView &, Ix64, unsigned int *, uint64_t);
template int sdti::host_index<Ix64, unsigned long long>(const GraphView &, Ix64, unsigned long long *, uint64_t);
