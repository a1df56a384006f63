"""The engine options the GPU tests run on.  The engine is one per process (get_engine caches it) and td_engine_set_option values outlive the
test that set them, so a test that leaves an option off its default moves every later test of the run onto a plan no user gets.  This module

  * reads the defaults that ship from the source itself (SHIPPED: the names in kKnownOptions of csrc/engine.hip, each with the literal of its
    `option("name", literal)` read sites; an option the engine only stores for the host samplers -- include/td_engine.h: "grid_fused" -- has its
    read sites, `get_option("name", literal)`, in the package's Python files),
  * gives the tests one way to change an option, pinned(), which puts back what was there before, and
  * brings an autouse fixture, engine_options_guard, into every GPU test module that imports it: before a GPU test and after it the options of
    every engine of the process are as shipped, "async" and "profile" included, or the test fails naming the options that are not.  The guard
    resets nothing: after a leak every later test fails its before-check too, each naming the same option, and the first one that failed its
    after-check is the one that leaks."""
import ast
import contextlib
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_HIP = os.path.join(ROOT, "terrain_diffusion_amd", "csrc", "engine.hip")
_LITERAL = r"([-+~0-9a-fA-FxXuUlL<>*\s]+?)"


def _strip_comments(text):
    """comments blanked, line breaks kept (the line numbers in the messages stay those of the file)"""
    return re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n") or " ", re.sub(r"//[^\n]*", " ", text), flags=re.S)


def _eval_literal(text, where):
    """an integer literal expression of C (`-1`, `65536`, `1 << 30`, `0x10`, `12LL`) as a Python int; anything else raises"""
    src = re.sub(r"(?<=[0-9a-fA-F])[uUlL]+\b", "", text.strip())

    def ev(n):
        if isinstance(n, ast.Constant) and type(n.value) is int:
            return n.value
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, (ast.USub, ast.UAdd, ast.Invert)):
            v = ev(n.operand)
            return -v if isinstance(n.op, ast.USub) else ~v if isinstance(n.op, ast.Invert) else v
        if isinstance(n, ast.BinOp) and isinstance(n.op, (ast.LShift, ast.RShift, ast.Mult, ast.Add, ast.Sub)):
            a, b = ev(n.left), ev(n.right)
            return {ast.LShift: a << b, ast.RShift: a >> b, ast.Mult: a * b, ast.Add: a + b, ast.Sub: a - b}[type(n.op)]
        raise ValueError(f"{where}: default {text!r} is not an integer literal expression")
    try:
        return ev(ast.parse(src, mode="eval").body)
    except SyntaxError:
        raise ValueError(f"{where}: default {text!r} is not an integer literal expression") from None


def parse_shipped(engine_src, host_srcs=()):
    """{option: default} from the text of engine.hip and of the host sources that read options (`host_srcs`: (name, text) pairs).  Raises when
    a name of kKnownOptions has no read site, has read sites with different defaults, or when a read site names an option that is not known."""
    src = _strip_comments(engine_src)
    m = re.search(r"kKnownOptions\s*\[\s*\]\s*=\s*\{(.*?)\}\s*;", src, flags=re.S)
    if not m:
        raise ValueError("engine.hip: no kKnownOptions table")
    known = re.findall(r'"([^"]+)"', m.group(1))
    if len(set(known)) != len(known):
        raise ValueError(f"kKnownOptions lists an option twice: {sorted(k for k in set(known) if known.count(k) > 1)}")
    sites = {}   # option -> {default: [where, ...]}
    for mm in re.finditer(r'\boption\(\s*"([^"]+)"\s*,\s*' + _LITERAL + r"\s*\)", src):
        where = f"engine.hip:{src.count(chr(10), 0, mm.start()) + 1}"
        sites.setdefault(mm.group(1), {}).setdefault(_eval_literal(mm.group(2), where), []).append(where)
    # a read site whose default is no literal (a variable, a call) must not pass for "no read site"
    for mm in re.finditer(r'\boption\(\s*"([^"]+)"\s*,', src):
        if mm.group(1) not in sites:
            raise ValueError(f'engine.hip: option("{mm.group(1)}", ...) is read with a default that is not an integer literal')
    for name, text in host_srcs:
        for mm in re.finditer(r'\bget_option\(\s*"([^"]+)"\s*,\s*' + _LITERAL + r"\s*\)", text):
            sites.setdefault(mm.group(1), {}).setdefault(_eval_literal(mm.group(2), name), []).append(name)
    unknown = sorted(set(sites) - set(known))
    if unknown:
        raise ValueError(f"read sites of options that kKnownOptions does not list: {unknown}")
    missing = [k for k in known if k not in sites]
    if missing:
        raise ValueError(f"known options without a read site (no default to learn): {missing}")
    split = {k: v for k, v in sites.items() if len(v) > 1}
    if split:
        raise ValueError(f"options read with different defaults: {split}")
    return {k: next(iter(sites[k])) for k in known}


def _load():
    host = []
    for f in sorted(glob.glob(os.path.join(ROOT, "terrain_diffusion_amd", "*.py"))):
        with open(f) as fh:
            host.append((os.path.relpath(f, ROOT), fh.read()))
    with open(ENGINE_HIP) as fh:
        return parse_shipped(fh.read(), host)


SHIPPED = _load()


def snapshot(eng):
    """{option: current value} of every known option"""
    return {k: eng.get_option(k, SHIPPED[k]) for k in SHIPPED}


def off_default(eng):
    return {k: v for k, v in snapshot(eng).items() if v != SHIPPED[k]}


def assert_shipped(eng, where):
    off = off_default(eng)
    assert not off, f"{where}: engine options off their shipped defaults: " + ", ".join(f"{k} = {v} (ships {SHIPPED[k]})" for k, v in sorted(off.items()))


@contextlib.contextmanager
def pinned(eng, **opts):
    """Set engine options for the body and put back the values they had BEFORE (not the defaults: blocks nest), exceptions included."""
    bad = sorted(k for k in opts if k not in SHIPPED)
    if bad:
        raise KeyError(f"not engine options: {bad}")
    before = {k: eng.get_option(k, SHIPPED[k]) for k in opts}
    try:
        for k, v in opts.items():
            eng.set_option(k, int(v))
        yield eng
    finally:
        for k, v in reversed(list(before.items())):
            eng.set_option(k, v)


def _live_engines():
    """the engines this process has created (none before the first get_engine: nothing can be off its default then)"""
    from terrain_diffusion_amd import engine as E
    return [e for _, e in sorted(E._engines.items()) if e._h]


def guard(engines, name):
    """the body of engine_options_guard as a plain generator (tests/test_engine_opts_cpu.py drives it with a stub engine)"""
    for e in engines():
        assert_shipped(e, f"before {name}")
    yield
    for e in engines():
        assert_shipped(e, f"after {name} (this test leaks them)")


@pytest.fixture(autouse=True)
def engine_options_guard(request):
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    yield from guard(_live_engines, request.node.nodeid)
