"""The grouped penalty of the multinomial Newton modes on the CPU: the option "mnewton_grouped", plan_fit's rung for
type_multinomial = 1 with and without FitFacts::grouped_newton (csrc/fit_plan.hpp, compiled with g++), the LDS bytes of the
two grouped inner solves restated (csrc/mnewton.hpp), and the numpy reference's own convergence on the GPU test's shapes."""
import pytest

import mnewton_grouped_reference as gr
import test_direct_plan_host as dp

MNEWTON, WMNEWTON, LDS_BYTES = 6, 10, 160 * 1024
LIMIT = {MNEWTON: lambda K: max(199 // K - 1, 0), WMNEWTON: lambda K: 5820 // K - 1}


def test_option_defaults_to_zero_and_takes_zero_or_one():
    import sgdnet_amd as sa
    assert sa.get_option("mnewton_grouped") == 0
    with sa.option("mnewton_grouped", 1):
        assert sa.get_option("mnewton_grouped") == 1
    for value in (-1, 2):
        with pytest.raises(sa.SgdnetError):
            sa.set_option("mnewton_grouped", value)
    assert sa.get_option("mnewton_grouped") == 0 and sa.get_option("mnewton_width") == 0
    for fit in (sa.sgdnet_mnewton, sa.sgdnet_wmnewton):                  # (refused before the native call)
        with pytest.raises(ValueError):
            fit(*gr.problem(60, 1, 2), type_multinomial="both")


PROGRAM = '''#include "fit_plan.hpp"
#include <cstdio>
using namespace sgdnet;
int main() {
  for (int grouped = 0; grouped < 2; ++grouped)
    for (int mode : {%d, %d})
      for (int K : {2, 3, 99})
        for (int at_limit = 0; at_limit < 2; ++at_limit) {
          sgdnet_control c{};
          c.mode = mode; c.family = SGDNET_MULTINOMIAL; c.n_classes = K; c.type_multinomial = 1; c.elasticnet_mix = 0.5;
          FitFacts f;
          f.ctl = &c; f.n = 100; f.n_devices = 1; f.grouped_newton = grouped != 0;
          f.p = !at_limit ? 1 : mode == SGDNET_MODE_MNEWTON ? mnewton_max_features(K) : wmnewton_max_features(K);
          const FitPlan P = plan_fit(f);
          printf("%%d %%d %%d %%lld\\t%%d\\t%%d\\t%%s\\n", grouped, mode, K, (long long)f.p, P.rc, P.penalty, P.error.c_str());
        }
  for (int K = 2; K <= 99; ++K)
    printf("lds %%d %%d %%d\\n", K, mnewton_max_features(K) > 0 ? 8 * mnewton_grouped_state_doubles(mnewton_max_features(K), K) : 0,
           wmnewton_grouped_state_bytes(wmnewton_max_features(K), K));
  return 0;
}
''' % (MNEWTON, WMNEWTON)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return dp.compile_and_run(str(tmp_path_factory.mktemp("grouped")), "grouped_plans", PROGRAM).split("\n")


def test_plan_takes_grouped_iff_the_fact_says_so(program):
    plans = [l.split("\t") for l in program if l and not l.startswith("lds")]
    assert len(plans) == 2 * 2 * 3 * 2
    for key, rc, penalty, msg in plans:
        grouped, mode, K, p = [int(v) for v in key.split()]
        assert p in (1, LIMIT[mode](K))
        if grouped:
            assert (int(rc), int(penalty), msg) == (0, 2, "")                     # SGDNET_GROUPLASSO
        else:                                                                     # the text of tests/golden/direct_plan_refusals.tsv
            assert int(rc) == -5 and msg == ("mode = %s needs the ungrouped penalty (type_multinomial = 0): family 2, n_classes %d, 100 samples, "
                                             "%d features (limit %d), n_gpus 0, debug 0" % ({MNEWTON: "mnewton", WMNEWTON: "wmnewton"}[mode], K, p, LIMIT[mode](K)))


def test_grouped_lds_layouts_fit_at_every_limit(program):
    rows = [[int(v) for v in l.split()[1:]] for l in program if l.startswith("lds")]
    assert [r[0] for r in rows] == list(range(2, 100))
    for K, narrow, wide in rows:
        p, pw = LIMIT[MNEWTON](K), LIMIT[WMNEWTON](K)
        Q, Qw, E = K * (p + 1), K * (pw + 1), pw + K
        # narrow: the triangle, U, g, t_j, the change scales and the block's steps; wide: g | U | T | S | d, then the list of blocks and intercepts
        assert narrow == 8 * (Q * (Q + 1) // 2 + 2 * Q + 2 * p + K) and narrow <= LDS_BYTES
        assert wide == 8 * (2 * Qw + E + pw + K) + 4 * E + 4 * ((E + 31) // 32) + 128
        assert wide <= 24 * Qw + 4 * Qw + 4 * ((Qw + 31) // 32) + 128 <= LDS_BYTES      # within the ungrouped wide layout's bytes


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("mix", gr.MIXES)
@pytest.mark.parametrize("shape", gr.SHAPES + gr.WIDE_ONLY)
def test_reference_converges_on_the_gpu_shapes(shape, mix, intercept):
    x, y = gr.problem(*shape)
    z = gr.standardised(x)[0]
    solved = gr.solve(z, y, shape[2], gr.user_lambdas(z, y, shape[2], mix, intercept), mix, intercept)
    assert max(res for _, _, res in solved) <= gr.FLOOR
    assert abs(solved[0][0]).max() < 1e-12                                    # lambda_max: nothing, or rounding
    assert (abs(solved[-1][0]).sum(1) > 0).sum() >= min(shape[1], 4)          # the path's end is not trivial
