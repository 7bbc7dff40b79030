#define FZ_R 4
#define FZ_AT fz::bf16
#define FZ_AT_TAG _bf16_cdsmu
#define FZ_NMF_CD_SMU 1
#include "nmf_kernels.inc"
