// udf_mlp_bf16x3.hip: the fused UDF-MLP kernels (udf_mlp_kernel.inc) and their launchers for EMAP_PREC_BF16X3.
#include "udf_mlp_kernel.inc"
namespace emap {
const MlpUnit* mlp_unit_bf16x3() { return mlp_unit_of<EMAP_PREC_BF16X3>(); }
}
