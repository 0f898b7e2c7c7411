// A stand-in for libeaofusion_hip.so's Initializer entry point that needs no device: it prints the call it receives and answers by a made-up rule, so that the CPU
// suite can check what include/eaofusion/Initializer.h sends and what it does with the answer.  The rule reads sigma:
//   sigma < 1.5   returned, branch F: R21[k] = k + 1, t21[k] = 10 + k, p3d[i] = (i, 2 i, 3 i), triangulated[i] = i % 3 == 0
//   sigma < 2.5   not returned, branch F        sigma < 3.5   not returned, branch H        otherwise   no_model
// tests/test_initializer_class_cpu.py restates it.
#include <cstdio>

#include <eao_fusion.h>

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_initializer_initialize(const eao_initializer_problem* p, const int32_t* sets, int32_t iterations, eao_initializer_result* r) {
    printf("call n1 %d n2 %d N %d K %.9g %.9g %.9g %.9g sigma %.9g minparallax %.9g mintri %d iterations %d keys1", p->n1, p->n2, p->n_matches, p->fx, p->fy, p->cx, p->cy,
           p->sigma, p->min_parallax, p->min_triangulated, iterations);
    for (int i = 0; i < 2 * p->n1; i++) printf(" %.9g", p->keys1_xy[i]);
    printf(" keys2");
    for (int i = 0; i < 2 * p->n2; i++) printf(" %.9g", p->keys2_xy[i]);
    printf(" matches");
    for (int i = 0; i < 2 * p->n_matches; i++) printf(" %d", p->matches12[i]);
    printf(" sets");
    for (int k = 0; k < 8 * iterations; k++) printf(" %d", sets[k]);
    printf("\n");
    r->returned = p->sigma < 1.5f;
    r->branch = p->sigma < 2.5f ? EAO_INIT_BRANCH_F : EAO_INIT_BRANCH_H;
    r->no_model = !(p->sigma < 3.5f);
    if (r->returned) {
        for (int k = 0; k < 9; k++) r->R21[k] = 1.f + k;
        for (int k = 0; k < 3; k++) r->t21[k] = 10.f + k;
        for (int i = 0; i < p->n1; i++) {
            r->p3d[3 * i] = (float)i; r->p3d[3 * i + 1] = 2.f * i; r->p3d[3 * i + 2] = 3.f * i;
            r->triangulated[i] = i % 3 == 0;
        }
    }
    return EAO_OK;
}

}  // extern "C"
