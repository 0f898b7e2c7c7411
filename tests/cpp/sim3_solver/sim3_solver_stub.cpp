// A stand-in for libeaofusion_hip.so's Sim3Solver entry point that needs no device: it prints every call it receives and answers with a made-up but
// rule-abiding result, so that the CPU suite can check what include/eaofusion/Sim3Solver.h sends and what it does with the answer.
//   count of hypothesis h = (7 t0 + 3 t1 + t2) % (n + 1); its flags: the first `count` correspondences; its T12[k] = 100 h + k.
// The sequential rule is the library's (src/Sim3Solver.cc:183-206); tests/test_sim3_solver_class_cpu.py restates both.
#include <algorithm>
#include <cstdio>

#include <eao_fusion.h>

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_sim3_solver_iterate(const eao_sim3_solver_problem* p, int32_t min_inliers, int32_t max_its, eao_sim3_solver_state* state, const int32_t* triples,
                                   int32_t n_hyp, eao_sim3_solver_result* r) {
    printf("call n %d fix %d min %d max %d iterations %d nhyp %d sigma", p->n, p->fix_scale, min_inliers, max_its, state->iterations, n_hyp);
    for (int i = 0; i < p->n; i++) printf(" %.9g/%.9g", p->sigma2_1[i], p->sigma2_2[i]);
    printf(" xw1");
    for (int i = 0; i < p->n; i++) printf(" %.9g", p->Xw1[3 * i]);
    printf(" triples");
    for (int k = 0; k < 3 * n_hyp; k++) printf(" %d", triples[k]);
    printf("\n");
    r->returned = -1; r->n_inliers = 0; r->no_more = 0;
    for (int k = 0; k < 16; k++) r->T12[k] = 0;
    if (p->n < min_inliers) { r->no_more = 1; return EAO_OK; }
    const int n_eval = std::max(0, std::min(n_hyp, max_its - state->iterations));
    for (int h = 0; h < n_eval; h++) {
        state->iterations++;
        const int count = (7 * triples[3 * h] + 3 * triples[3 * h + 1] + triples[3 * h + 2]) % (p->n + 1);
        if (count >= state->best_inliers) {
            state->best_inliers = count;
            for (int k = 0; k < 16; k++) state->best_T12[k] = 100.f * h + k;
            for (int k = 0; k < 9; k++) state->best_R[k] = 10.f * h + k;
            for (int k = 0; k < 3; k++) state->best_t[k] = 1000.f * h + k;
            state->best_s = 1.f + h;
            if (count > min_inliers) {
                r->returned = h; r->n_inliers = count;
                for (int k = 0; k < 16; k++) r->T12[k] = state->best_T12[k];
                for (int i = 0; i < p->n; i++) r->inlier[i] = i < count;
                return EAO_OK;
            }
        }
    }
    if (state->iterations >= max_its) r->no_more = 1;
    return EAO_OK;
}

eao_status eao_optimize_sim3(const eao_sim3_problem*, eao_sim3_result*) { return EAO_ERR_NO_DEVICE; }

}  // extern "C"
