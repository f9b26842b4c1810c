// udf_mlp_f16.hip: the fused UDF-MLP kernels (udf_mlp_kernel.inc) and their launchers for EMAP_PREC_F16.
#include "udf_mlp_kernel.inc"
namespace emap {
const MlpUnit* mlp_unit_f16() { return mlp_unit_of<EMAP_PREC_F16>(); }
}
