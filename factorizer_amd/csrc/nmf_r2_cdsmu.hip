#define FZ_R 2
#define FZ_AT float
#define FZ_AT_TAG _cdsmu
#define FZ_NMF_CD_SMU 1
#include "nmf_kernels.inc"
