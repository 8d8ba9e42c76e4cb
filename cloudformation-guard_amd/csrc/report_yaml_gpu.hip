// The device YAML report writer: report_gpu.hip's record walk compiled with the block-YAML writer (rg::Y)
// as report_yaml_kernel.  Same source, GG_REPORT_YAML 1; a unit of its own so it builds beside the JSON /
// SARIF kernels and leaves their code as it was.
#define GG_REPORT_YAML 1
#include "report_gpu.hip"
