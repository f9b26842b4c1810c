// udf_mlp_f16x3.hip: the fused UDF-MLP kernels (udf_mlp_kernel.inc) and their launchers for EMAP_PREC_F16X3.
#include "udf_mlp_kernel.inc"
namespace emap {
const MlpUnit* mlp_unit_f16x3() { return mlp_unit_of<EMAP_PREC_F16X3>(); }
}
#ifdef EMAP_TIMELINE      // probe builds only
extern "C" int emap_debug_fs2_timeline(long long* dst, int n) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(emap::emap_ftl_buf), (size_t)n * sizeof(long long));
}
#endif
