/* Diagnostic-build additions to the C ABI (libldmae_hip_diag.so, `make -C ldmae_amd/csrc diag`).  NOT part of the product
 * library or of include/ldmae_hip.h: process-wide A/B knobs and the tile-timeline stamp buffer used by tools/ (bench_nt.py,
 * gemm_timeline.py, gap_probe.py, one_gemm.py).  Select the library with LDMAE_HIP_LIB=<repo>/ldmae_amd/libldmae_hip_diag.so. */
#ifndef LDMAE_DIAG_H
#define LDMAE_DIAG_H
#ifdef __cplusplus
extern "C" {
#endif
/* kernel-variant selection for A/B measurements.  The live keys (the list itself is in core.hip): 1: 1 = the 128 x 128 TN kernel,
 * 5: NT start delay, 7: 1 = per-K-step stamp build, 8: NT launch mode (2 = one tile per workgroup; the product library takes this per call
 * through LDMAE_EPI_TILE_LAUNCH), 9: TN split target, 10: row-kernel grid cap, 11: launch-gap probes (1 = empty kernel, 2 = ntiles = 0),
 * 16: NT column-group tile walk (column tiles per group), 19: 1 = the half-line NT kernel, 23 / 24: operand-fragment prefetch depth of the
 * fused (QK-norm) attention backward's dK/dV / dQ kernel (attention.hip: 1 / 2 = that depth, 3 = none), 25: the same for the plain
 * dQ + dK/dV pair (1 = depth 1, 3 = none).
 * 0 = shipped behaviour.  Any other key, retired (tools/README.md) or never assigned, is refused with LDMAE_ERR_INVALID. */
int ldmae_tune(int key, int value);
int ldmae_tune_query(int key);
/* device buffer (>= 64 B x 256 workgroups x tiles-per-workgroup) that receives s_memrealtime stamps of the persistent NT GEMM
 * (tile start / main loop end / epilogue issued / stores drained); NULL (default) = off */
void ldmae_debug_nt_stamps(void* buf);
#ifdef __cplusplus
}
#endif
#endif
