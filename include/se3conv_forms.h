/* libse3conv_hip.so: which kernel form every launch of the fused operator takes -- a host-only query.
 *
 * This header is an addition inside SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged. */
#ifndef SE3CONV_FORMS_H
#define SE3CONV_FORMS_H

#include "se3conv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which kernel forms a call would launch (host only, touches no device).  se3conv_fwd and
 * se3conv_bwd do not run one kernel each: every launcher picks one of several template instantiations from the shape
 * (channel widths, frame counts, row format, sizes), and this query walks the call's own stage sequence with every launch
 * replaced by its launcher's decision -- there is no second copy of the conditions.  `pass`: SE3_PASS_FWD (`have_t` = the
 * call keeps T, t_save != NULL; want_* ignored) or SE3_PASS_BWD with the request as se3conv_bwd_workspace_bytes takes it
 * (want_params = all three parameter gradients).  `cu_count`: compute units of the device the call would run on (>= 1;
 * resident grids, and with them a few forms, are sized by it: 256 on an MI355X).  Writes one "stage:form\n" line per
 * launch that carries a profile tag (se3_profile_read), in launch order, NUL-terminated, e.g.
 *   edge_t_fwd:edge_t_pair<ct=2,full=0,nf=1,p2=0,tr=-1>/fmt1        gemm_out:gemm_nn_t24<mode=2,nb=2>
 *   edge_param_grad:param_grad_pair<ch16=4,p2=1>/pipe/y3            reductions:reduce_batch/a+s+w
 * A launch inside another's stage (the reduction behind a split GEMM) is a line of its own under that stage.  For
 * num_basis != 32 the lines are those of the inner K = 32 calls, slice after slice.  The SE3_* environment switches act on
 * the answer exactly as on the launches (both read them once per process).  Returns SE3_OK, SE3_ERR_WORKSPACE when `len`
 * is too small, or what the call itself would return for the shape. */
#define SE3_PASS_FWD 0
#define SE3_PASS_BWD 1
int se3conv_forms(const se3conv_shape* shape, int pass, int want_feat, int want_params, int have_t, int cu_count, char* buf,
                  size_t len);

#ifdef __cplusplus
}
#endif

#endif  /* SE3CONV_FORMS_H */
