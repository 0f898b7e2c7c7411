// A stand-in for libeaofusion_hip.so's PnPsolver entry point that needs no device: it prints every call it receives and answers with a made-up but rule-abiding
// result, so that the CPU suite can check what include/eaofusion/PnPsolver.h sends and what it does with the answer.
//   count of hypothesis h = (sum over i of (i + 1) * set[i]) % (n + 1); its flags: the first `count` correspondences; its Tcw[k] = 100 count + k.
//   Refine of a set of c correspondences ends with c + 1 inliers (capped at n) when c % 3 == 0, else with c; its flags: the first that many; Tcw[k] = -(100 c + k).
// The sequential rule is the library's (src/PnPsolver.cc:182-255, Refine at every gate-passing hypothesis); tests/test_pnp_solver_class_cpu.py restates both.
#include <algorithm>
#include <cstdio>

#include <eao_fusion.h>

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_pnp_solver_iterate(const eao_pnp_solver_problem* p, int32_t min_inliers, int32_t max_its, int32_t min_set, eao_pnp_solver_state* state,
                                  const int32_t* sets, int32_t n_hyp, eao_pnp_solver_result* r) {
    printf("call n %d min %d max %d set %d iterations %d best %d nhyp %d th2 %.9g K %.9g %.9g %.9g %.9g sigma", p->n, min_inliers, max_its, min_set, state->iterations,
           state->best_inliers, n_hyp, p->th2, p->fx, p->fy, p->cx, p->cy);
    for (int i = 0; i < p->n; i++) printf(" %.9g", p->sigma2[i]);
    printf(" x");
    for (int i = 0; i < p->n; i++) printf(" %.9g", p->p3d_w[3 * i]);
    printf(" u");
    for (int i = 0; i < p->n; i++) printf(" %.9g", p->p2d[2 * i]);
    printf(" sets");
    for (int k = 0; k < min_set * n_hyp; k++) printf(" %d", sets[k]);
    printf("\n");
    r->returned = -1; r->refined = 0; r->n_inliers = 0; r->no_more = 0; r->n_records = 0;
    for (int k = 0; k < 16; k++) r->Tcw[k] = 0;
    if (p->n < min_inliers) { r->no_more = 1; return EAO_OK; }
    int best_hyp = -1;
    for (int h = 0; h < n_hyp; h++) {
        state->iterations++;
        long s = 0;
        for (int i = 0; i < min_set; i++) s += (long)(i + 1) * sets[h * min_set + i];
        const int count = (int)(s % (p->n + 1));
        if (count >= min_inliers) {
            if (count > state->best_inliers) {
                state->best_inliers = count;
                best_hyp = h;
                for (int k = 0; k < 16; k++) state->best_Tcw[k] = 100.f * count + k;
                for (int i = 0; i < p->n; i++) state->best_inlier[i] = i < count;
            }
            const int c = state->best_inliers;
            const int refined = std::min(p->n, c + (c % 3 == 0 ? 1 : 0));
            if (refined > min_inliers) {
                r->returned = h; r->refined = 1; r->n_inliers = refined;
                for (int k = 0; k < 16; k++) r->Tcw[k] = -(100.f * c + k);
                for (int i = 0; i < p->n; i++) r->inlier[i] = i < refined;
                return EAO_OK;
            }
        }
    }
    if (state->iterations >= max_its) {
        r->no_more = 1;
        if (state->best_inliers >= min_inliers) {
            r->returned = best_hyp >= 0 ? best_hyp : n_hyp; r->n_inliers = state->best_inliers;
            for (int k = 0; k < 16; k++) r->Tcw[k] = state->best_Tcw[k];
            for (int i = 0; i < p->n; i++) r->inlier[i] = state->best_inlier[i];
        }
    }
    return EAO_OK;
}

eao_status eao_pose_optimization(const eao_pose_problem*, eao_pose_result*) { return EAO_ERR_NO_DEVICE; }

}  // extern "C"
