// udf_mlp_bf16.hip: the fused UDF-MLP kernels (udf_mlp_kernel.inc) and their launchers for EMAP_PREC_BF16.
#include "udf_mlp_kernel.inc"
namespace emap {
const MlpUnit* mlp_unit_bf16() { return mlp_unit_of<EMAP_PREC_BF16>(); }
}
