"""tests/_engine_opts.py without a GPU: the defaults it reads from csrc/engine.hip, and pinned() / the guard against a stub engine."""
import re

import pytest

import _engine_opts as eo


class StubEngine:
    """a dict behind set_option / get_option, as td_engine_set_option / td_engine_get_option keep one"""

    def __init__(self, **opt):
        self.opt = dict(opt)

    def set_option(self, key, value):
        self.opt[key] = int(value)

    def get_option(self, key, default):
        return self.opt.get(key, int(default))


def _known_options():
    """the names between the braces of kKnownOptions, read here a second time and more bluntly: every quoted word of those lines"""
    text = open(eo.ENGINE_HIP).read()
    body = text[text.index("kKnownOptions[] = {"):]
    body = body[:body.index("};")]
    return re.findall(r'"(\w+)"', re.sub(r"//[^\n]*", "", body))


def test_parse_covers_exactly_the_known_options_with_one_default_each():
    known = _known_options()
    assert len(known) >= 50 and len(set(known)) == len(known)
    assert list(eo.SHIPPED) == known
    assert all(type(v) is int for v in eo.SHIPPED.values())


def test_spot_values():
    s = eo.SHIPPED
    assert s["dual_stream"] == 1 and s["glds_min_wgs"] == 8 and s["plan_cache_max"] == 12 and s["sb_max_glds_wgs"] == 1 << 30
    assert s["dual_stream_min_batch"] == 32 and s["solver_order"] == 2 and s["lower_order_final"] == 1 and s["sampler_stop_after"] == -1
    assert s["async"] == 0 and s["profile"] == 0 and s["batch_invariant"] == 0 and s["plan_cache_mb"] == 65536 and s["grid_fused"] == 1


SRC = 'static const char* const kKnownOptions[] = {\n  // first\n  "a", "b"};\nx = e->option("a", 1 << 4); /* option("b", 9) */ y = u->eng->option("b", -1); z = e->option("a", 16);\n'


def test_parser_on_a_small_source():
    assert eo.parse_shipped(SRC) == {"a": 16, "b": -1}
    assert eo.parse_shipped(SRC.replace('u->eng->option("b", -1)', "0"), [("host.py", 'eng.get_option("b", 3) != 0')]) == {"a": 16, "b": 3}


def test_parser_refuses_a_known_option_without_a_read_site():
    with pytest.raises(ValueError, match=r"without a read site.*'b'"):
        eo.parse_shipped(SRC.replace('u->eng->option("b", -1)', "0"))


def test_parser_refuses_two_read_sites_with_different_defaults():
    with pytest.raises(ValueError, match="different defaults.*'a'"):
        eo.parse_shipped(SRC.replace('option("a", 16)', 'option("a", 15)'))
    with pytest.raises(ValueError, match="different defaults.*'b'"):
        eo.parse_shipped(SRC, [("host.py", 'eng.get_option("b", 3)')])


def test_parser_refuses_a_read_site_it_cannot_evaluate_or_does_not_know():
    with pytest.raises(ValueError, match="not an integer literal"):
        eo.parse_shipped(SRC.replace('option("b", -1)', 'option("b", kDefault)'))
    with pytest.raises(ValueError, match="does not list.*'c'"):
        eo.parse_shipped(SRC + 'w = e->option("c", 0);\n')


def test_snapshot_and_assert_shipped():
    eng = StubEngine()
    assert eo.snapshot(eng) == eo.SHIPPED
    eo.assert_shipped(eng, "fresh")
    eng.set_option("glds_min_wgs", 192); eng.set_option("dual_stream", 0); eng.set_option("sb", 1)   # sb = 1 is the default, set explicitly
    with pytest.raises(AssertionError) as ei:
        eo.assert_shipped(eng, "here")
    msg = str(ei.value)
    assert "here" in msg and "glds_min_wgs = 192 (ships 8)" in msg and "dual_stream = 0 (ships 1)" in msg and "sb =" not in msg


def test_pinned_restores_prior_values_after_an_exception():
    eng = StubEngine()
    with pytest.raises(RuntimeError, match="boom"):
        with eo.pinned(eng, dual_stream=0, glds_min_wgs=192, profile=1):
            assert (eng.get_option("dual_stream", 1), eng.get_option("glds_min_wgs", 8), eng.get_option("profile", 0)) == (0, 192, 1)
            raise RuntimeError("boom")
    eo.assert_shipped(eng, "after the exception")


def test_pinned_restores_a_non_default_value_to_that_value():
    eng = StubEngine(dual_stream=0)
    with eo.pinned(eng, dual_stream=1, dual_stream_min_batch=2):
        with eo.pinned(eng, dual_stream_min_batch=7):
            assert eng.get_option("dual_stream_min_batch", 32) == 7
        assert eng.get_option("dual_stream", 1) == 1 and eng.get_option("dual_stream_min_batch", 32) == 2
    assert eng.get_option("dual_stream", 1) == 0 and eng.get_option("dual_stream_min_batch", 32) == 32
    assert eo.off_default(eng) == {"dual_stream": 0}


def test_pinned_refuses_an_unknown_key_and_sets_nothing():
    eng = StubEngine()
    with pytest.raises(KeyError, match="batch_invarient"):
        with eo.pinned(eng, dual_stream=0, batch_invarient=1):
            pass
    assert eng.opt == {}


def _run_guarded(eng, body):
    g = eo.guard(lambda: [eng], "test_x")
    next(g)          # the before-check
    body()
    with pytest.raises(StopIteration):
        next(g)      # the after-check


def test_guard_names_the_option_a_body_leaks():
    eng = StubEngine()
    with pytest.raises(AssertionError, match=r"after test_x.*leaks.*dual_stream = 0 \(ships 1\)"):
        _run_guarded(eng, lambda: eng.set_option("dual_stream", 0))
    # and the next test's before-check sees it too: nothing was reset behind anybody's back
    with pytest.raises(AssertionError, match=r"before test_x.*dual_stream = 0"):
        next(eo.guard(lambda: [eng], "test_x"))


def test_guard_sees_async_and_profile():
    for key in ("async", "profile"):
        eng = StubEngine()
        with pytest.raises(AssertionError, match=rf"{key} = 1 \(ships 0\)"):
            _run_guarded(eng, lambda: eng.set_option(key, 1))


def test_guard_passes_when_nothing_leaks():
    eng = StubEngine()

    def body():
        with eo.pinned(eng, glds_min_wgs=192):
            pass
    _run_guarded(eng, body)
    _run_guarded(StubEngine(), lambda: None)
    g = eo.guard(lambda: [], "test_x")    # no engine yet in the process
    next(g)
    with pytest.raises(StopIteration):
        next(g)
