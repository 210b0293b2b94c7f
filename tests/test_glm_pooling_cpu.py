"""Per-response stepsize and metric of a GLM with several responses (IDHMC_EPS_PER_RESPONSE, IDHMC_METRIC_PER_RESPONSE; DESIGN
section 16), the part that needs no device: the constants, and every refusal of the creation path with the offending value in its
message.  Every check answers before the device is looked for; the rows are built like those of tests/test_create_refusals_cpu.py
(valid rows expect a context, or "no HIP device", which is past every argument check)."""
import numpy as np
import pytest

from test_create_refusals_cpu import World

M, R = 5, 7


@pytest.fixture(scope="module")
def world(idhmc):
    w = World(idhmc)
    w.Y5 = np.stack([w.Ya + 0.125 * m * np.array([1.0, 0.0]) for m in range(M)])      # five planes, K = 2
    w.src = idhmc.glm.WEIBULL_LOG_LOGSHAPE.encode()
    return w


def test_the_constants_are_exported_and_default_options_carries_them(idhmc):
    assert (idhmc.EPS_PER_CHAIN, idhmc.EPS_GLOBAL, idhmc.EPS_PER_RESPONSE) == (0, 1, 2)
    assert (idhmc.METRIC_PER_CHAIN, idhmc.METRIC_SHARED, idhmc.METRIC_POOLED, idhmc.METRIC_PER_RESPONSE) == (0, 1, 2, 3)
    o = idhmc.default_options(eps_mode=idhmc.EPS_PER_RESPONSE, metric_mode=idhmc.METRIC_PER_RESPONSE)
    assert (o.eps_mode, o.metric_mode) == (2, 3)
    o = idhmc.default_options()
    assert (o.eps_mode, o.metric_mode) == (idhmc.EPS_PER_CHAIN, idhmc.METRIC_PER_CHAIN)
    import re
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idhmc.h")).read()
    assert re.search(r"IDHMC_EPS_PER_RESPONSE = 2\b", header) and re.search(r"IDHMC_METRIC_PER_RESPONSE = 3\b", header)


def modes(idhmc):
    """(name, options keywords) of the three ways to ask for pooling per response"""
    return (("eps", dict(eps_mode=idhmc.EPS_PER_RESPONSE)), ("metric", dict(metric_mode=idhmc.METRIC_PER_RESPONSE)),
            ("both", dict(eps_mode=idhmc.EPS_PER_RESPONSE, metric_mode=idhmc.METRIC_PER_RESPONSE)))


def ok(idhmc, rc, msg):
    return rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg)


def bad(idhmc, got, message):
    assert got == (idhmc.ERR_BAD_ARG, message), got


def test_a_valid_description_passes(world):
    idhmc = world.idhmc
    for name, kw in modes(idhmc):
        rc, msg = world.parts(M=M, R=R, Y=world.Y5, nchains=M * R, source=world.src, opt=world.opt(**kw))
        assert ok(idhmc, rc, msg), (name, rc, msg)
    # whole responses in the middle of the model; one response in one context (M = 1, any chains_per_response = nchains)
    rc, msg = world.parts(M=M, R=R, Y=world.Y5, nchains=2 * R, first=2 * R, source=world.src, opt=world.opt(**modes(idhmc)[2][1]))
    assert ok(idhmc, rc, msg), (rc, msg)
    rc, msg = world.parts(M=1, R=40, nchains=40, source=world.src, opt=world.opt(**modes(idhmc)[2][1]))
    assert ok(idhmc, rc, msg), (rc, msg)
    # a partial-response shard stays what it was in every other mode
    rc, msg = world.parts(M=M, R=R, Y=world.Y5, nchains=9, first=5, source=world.src)
    assert ok(idhmc, rc, msg), (rc, msg)


def test_a_misaligned_shard_is_refused(world):
    idhmc = world.idhmc
    for name, kw in modes(idhmc):
        word = b"metric_mode" if name == "metric" else b"eps_mode"
        bad(idhmc, world.parts(M=M, R=R, Y=world.Y5, nchains=R, first=5, opt=world.opt(**kw)),
            b"GLM_AUX: first_chain_id = 5 is not a multiple of chains_per_response = 7: a context with " + word +
            b" = PER_RESPONSE holds whole responses")
        bad(idhmc, world.parts(M=M, R=R, Y=world.Y5, nchains=9, first=0, opt=world.opt(**kw)),
            b"GLM_AUX: nchains = 9 is not a multiple of chains_per_response = 7: a context with " + word +
            b" = PER_RESPONSE holds whole responses")
    # a chain without a response is reported first, as in every other mode
    bad(idhmc, world.parts(M=M, R=R, Y=world.Y5, nchains=36, opt=world.opt(**modes(idhmc)[2][1])),
        b"GLM_AUX: first_chain_id + nchains = 36 is past the M * chains_per_response = 5 * 7 chains of the model")


def test_a_context_without_responses_is_refused(world):
    idhmc = world.idhmc
    eps, metric = world.opt(eps_mode=idhmc.EPS_PER_RESPONSE), world.opt(metric_mode=idhmc.METRIC_PER_RESPONSE)
    e_msg = b"eps_mode = 2 (PER_RESPONSE) needs a context made by idhmc_create_glm_responses"
    m_msg = b"metric_mode = 3 (PER_RESPONSE) needs a context made by idhmc_create_glm_responses"
    # idhmc_create_glm (a GLM in parts, M is None), idhmc_create with a packed GLM, a Gaussian
    bad(idhmc, world.parts(source=world.src, opt=eps), e_msg)
    bad(idhmc, world.parts(source=world.src, opt=metric), m_msg)
    bad(idhmc, world.packed(6, 7, world.aux, source=world.src, opt=eps), e_msg)
    bad(idhmc, world.packed(6, 7, world.aux, source=world.src, opt=metric), m_msg)
    bad(idhmc, world.packed(0, 4, opt=eps), e_msg)
    bad(idhmc, world.packed(0, 4, opt=metric), m_msg)
    # both asked for: the stepsize's is reported
    bad(idhmc, world.packed(0, 4, opt=world.opt(eps_mode=idhmc.EPS_PER_RESPONSE, metric_mode=idhmc.METRIC_PER_RESPONSE)), e_msg)


def test_the_metric_modes_known(world):
    idhmc = world.idhmc
    bad(idhmc, world.packed(0, 4, opt=world.opt(metric_mode=4)), b"unknown metric_mode 4")
    bad(idhmc, world.packed(0, 4, opt=world.opt(metric_mode=-1)), b"unknown metric_mode -1")
    bad(idhmc, world.packed(0, 4, opt=world.opt(metric_mode=7)), b"unknown metric_mode 7")
    bad(idhmc, world.parts(M=M, R=R, Y=world.Y5, nchains=M * R, opt=world.opt(metric_mode=4)), b"unknown metric_mode 4")


def test_the_per_response_metric_shares_the_per_chain_limit_on_D(world):
    idhmc = world.idhmc
    big = dict(X=np.ones((2, 510)), Y=np.zeros((2, 2, 1)), K=1, nc=0, constants=None, groups=[0, 1] * 255, M=2, R=3, nchains=6)    # D = 513
    bad(idhmc, world.parts(opt=world.opt(metric_mode=idhmc.METRIC_PER_RESPONSE), **big),
        b"GLM_AUX with D = 513 > 512 and metric_mode = PER_RESPONSE: the per-response metric is stored per chain and shares the "
        b"per-chain metric's LDS budget of the NUTS kernel (use SHARED)")
    bad(idhmc, world.parts(**big), b"GLM_AUX with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)")
    # the stepsize alone has no such limit: with the per-chain metric the refusal is the per-chain metric's
    bad(idhmc, world.parts(opt=world.opt(eps_mode=idhmc.EPS_PER_RESPONSE), **big),
        b"GLM_AUX with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)")


def test_the_context_wide_modes_are_refused_as_before(world):
    idhmc = world.idhmc
    bad(idhmc, world.parts(M=3, opt=world.opt(eps_mode=idhmc.EPS_GLOBAL)),
        b"GLM_AUX: M = 3 responses with eps_mode = GLOBAL: the global stepsize pools the acceptance of chains that sample different "
        b"posteriors (use PER_CHAIN)")
    bad(idhmc, world.parts(M=2, R=9, opt=world.opt(metric_mode=idhmc.METRIC_POOLED)),
        b"GLM_AUX: M = 2 responses with metric_mode = POOLED: the pooled metric pools the windows of chains that sample different "
        b"posteriors (use PER_CHAIN or SHARED)")
    # ... also next to a per-response mode of the other option
    bad(idhmc, world.parts(M=3, opt=world.opt(eps_mode=idhmc.EPS_GLOBAL, metric_mode=idhmc.METRIC_PER_RESPONSE)),
        b"GLM_AUX: M = 3 responses with eps_mode = GLOBAL: the global stepsize pools the acceptance of chains that sample different "
        b"posteriors (use PER_CHAIN)")
