"""Host side of the dimension tests (no GPU): the zero-extension premise of tests/dims_support.py on the numpy
oracle, the placements' coverage, and a scan of csrc's dimension dispatch: the one macro CBO_FOR_DIM, its uses, and the
``case N:`` lines that remain.

The oracle's BLAS may associate a dot product differently for another column count, so the oracle is compared at the
rtol tests/test_parity_gpu.py::test_ragged_sizes_and_dims applies (1e-7 mean, 1e-6 variance), not bit for bit; the
bit-for-bit statement is the device's (tests/test_dims_gpu.py).  A dummy column's gradient is an exact zero here too:
every term of it carries a factor (0 - 0).
"""
import glob
import os
import re

import numpy as np
import pytest

import dims_support as S
from oracle import gp_oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cbo_with_oop_amd", "csrc")
N, M = 130, 70


def test_placements_cover_every_slot():
    assert len(S.EMBEDDINGS) == 19
    for D in S.DIMS:
        pairs = S.placements(D)
        assert all(0 <= i < j < D for i, j in pairs) and len(set(pairs)) == len(pairs)
        assert {k for p in pairs for k in p} == set(range(D)), (D, pairs)
        assert any(i == 0 for i, _ in pairs) and any(i > 0 for i, _ in pairs)
    # D = 8 (dims_support.BIT_EMBEDDINGS): the adjacent pairs cover every slot too, the prefix (0, 1) and slots >= 4 included
    assert len(S.BIT_EMBEDDINGS) == 19 and S.TREE_EMBEDDINGS == [(8, p) for p in S.placements(8)]
    eight = [p for D, p in S.BIT_EMBEDDINGS if D == 8]
    assert (0, 1) in eight and {k for p in eight for k in p} == set(range(8))
    assert [e for e in S.BIT_EMBEDDINGS if e[0] < 8] == [e for e in S.EMBEDDINGS if e[0] < 8]


def test_embed_places_the_live_columns_and_zeros():
    A = np.arange(1.0, 7.0).reshape(3, 2)
    E = S.embed(A, 5, (1, 3))
    assert np.array_equal(E[:, [1, 3]], A) and np.all(E[:, [0, 2, 4]] == 0.0)
    ls = S.embed_lengthscales([0.9, 1.4], 5, (1, 3))
    assert np.array_equal(ls, [0.7 + 0.1 * 0, 0.9, 0.7 + 0.1 * 2, 1.4, 0.7 + 0.1 * 4]) and np.all(ls > 0)


def test_condition_bound_holds_and_is_small():
    """The bound is a condition; here it is checked once against a measured cond(Ky) and against the 3e4 the tests rely on."""
    for variant in S.VARIANTS:
        p = S.base_problem(300, 1, 0, variant)
        okw = S.oracle_kwargs(p)
        vmax = float(np.max(okw["vX"])) if p["causal"] else 0.0
        assert vmax <= 0.05 + 0.02 * 4.0
        bound = S.condition_bound(300, max_prior_var=0.05 + 0.02 * 4.0)
        assert bound < 4.5e4
        assert S.condition_bound(130, max_prior_var=0.13) < 3e4
        K = O.causal_K(p["X"], p["X"], okw.get("vX"), okw.get("vX"), p["variance"], p["lengthscale"], zero_diag=not p["causal"])
        K[np.diag_indices_from(K)] += p["noise_var"]
        assert np.linalg.cond(K) <= bound


@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("emb", S.EMBEDDINGS + [e for e in S.BIT_EMBEDDINGS if e[0] == 8], ids=S.embedding_id)
def test_embedding_premise_on_the_oracle(emb, variant):
    D, pos = emb
    p = S.base_problem(N, M, 11, variant)
    mXs, vXs = S.oracle_priors(p, p["Xs"])
    base = O.fit(p["X"], p["y"], **S.oracle_kwargs(p))
    post = O.fit(S.embed(p["X"], D, pos), p["y"], **S.oracle_kwargs(p, D, pos))
    assert base.tries == post.tries == 0
    Xs = S.embed(p["Xs"], D, pos)
    mu0, v0 = O.predict(base, p["Xs"], mXs, vXs)
    mu, v = O.predict(post, Xs, mXs, vXs)
    assert np.allclose(mu, mu0, rtol=1e-7, atol=1e-9) and np.allclose(v, v0, rtol=1e-6)
    assert np.allclose(post.L, base.L, rtol=1e-9, atol=1e-12) and np.allclose(post.alpha, base.alpha, rtol=1e-6, atol=1e-9)
    dm0, dv0 = O.predict_gradients(base, p["Xs"], vXs)
    dm, dv = O.predict_gradients(post, Xs, vXs)
    live, dummy = list(pos), S.dummies(D, pos)
    assert np.allclose(dm[:, live], dm0, rtol=1e-7, atol=1e-9 * np.max(np.abs(dm0)))
    assert np.allclose(dv[:, live], dv0, rtol=1e-6, atol=1e-9 * np.max(np.abs(dv0)))
    assert np.all(dm[:, dummy] == 0.0) and np.all(dv[:, dummy] == 0.0)
    g0 = O.log_marginal_likelihood_gradients(base)
    g = O.log_marginal_likelihood_gradients(post)
    scale = max(abs(g0[0]), np.max(np.abs(g0[1])), abs(g0[2]))
    assert np.isclose(O.log_marginal_likelihood(post), O.log_marginal_likelihood(base), rtol=1e-9)
    assert np.isclose(g[0], g0[0], rtol=1e-6, atol=1e-8 * scale) and np.isclose(g[2], g0[2], rtol=1e-6, atol=1e-8 * scale)
    if p["ard"]:
        assert np.allclose(g[1][live], g0[1], rtol=1e-6, atol=1e-8 * scale)
        assert np.all(g[1][dummy] == 0.0)
    else:
        assert g[1].shape == (1,) and np.allclose(g[1], g0[1], rtol=1e-6, atol=1e-8 * scale)


CASE = re.compile(r"^\s*case\s+(\d+)\s*:(.*)$")
TEMPLATE_ARG = re.compile(r"<\s*(\d+)\s*[,>]")
MACRO_ARG = re.compile(r"\b[A-Z][A-Z0-9_]*\(\s*(\d+)\s*\)")
D_ARG = re.compile(r"<\s*D\s*[,>]|\b[A-Z][A-Z0-9_]*\(\s*D\s*[,)]")
COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)
DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(CBO_FOR_DIM(?:_CASE)?)\((?:[^\n]*\\\n)*[^\n]*\n", re.M)


def csrc_sources():
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            yield os.path.basename(path), f.read()


def dispatch_uses(text):
    """(line, dimension expression, body) of every CBO_FOR_DIM(...) call in a text without comments and definitions"""
    for hit in re.finditer(r"\bCBO_FOR_DIM\(", text):
        depth, comma, at = 1, None, hit.end()
        while depth:
            c = text[at]
            depth += (c == "(") - (c == ")")
            if c == "," and depth == 1 and comma is None:
                comma = at
            at += 1
        assert comma is not None, text[hit.start():at]
        yield text.count("\n", 0, hit.start()) + 1, text[hit.end():comma].strip(), text[comma + 1:at - 1]


def test_every_case_label_launches_its_own_instantiation():
    """A dimension launched with another dimension's instantiation fails here before it reaches a GPU.

    ``case N:`` followed on the same line by a template argument list or an upper-case macro call whose first argument is
    a literal: that literal is N.  Only kernels_append.hip's two tile-count tables still have such lines; every dimension
    goes through CBO_FOR_DIM (cbo_device.h), whose helper writes N once, as the label and as D.  The macro is defined
    once, its helper is invoked for 1..7, each once, the default binds CBO_MAX_DIM, and every use instantiates with D and
    with no literal."""
    checked, wrong = {}, []
    for name, text in csrc_sources():
        for no, line in enumerate(text.splitlines(), 1):
            hit = CASE.match(line)
            if not hit:
                continue
            args = TEMPLATE_ARG.findall(hit.group(2)) + MACRO_ARG.findall(hit.group(2))
            if not args:
                continue
            checked[name] = checked.get(name, 0) + 1
            if any(int(a) != int(hit.group(1)) for a in args):
                wrong.append(f"{name}:{no}: {line.strip()}")
    assert not wrong, "\n".join(wrong)
    assert checked == {"kernels_append.hip": 6}, checked     # (switch (kp / 16): a tile count, not a dimension)

    defines, uses = {}, []
    for name, text in csrc_sources():
        text = COMMENT.sub("", text)
        for hit in DEFINE.finditer(text):
            defines.setdefault(hit.group(1), []).append(hit.group(0))
        rest = DEFINE.sub(lambda m: "\n" * m.group(0).count("\n"), text)       # (line numbers stay)
        uses += [(f"{name}:{no}", d, body) for no, d, body in dispatch_uses(rest)]
    assert {k: len(v) for k, v in defines.items()} == {"CBO_FOR_DIM": 1, "CBO_FOR_DIM_CASE": 1}, defines
    helper = " ".join(defines["CBO_FOR_DIM_CASE"][0].replace("\\\n", " ").split())
    assert helper == "#define CBO_FOR_DIM_CASE(N, ...) case N: { constexpr int D = N; __VA_ARGS__; } break;", helper
    macro = " ".join(defines["CBO_FOR_DIM"][0].replace("\\\n", " ").split())
    cases = "".join(f" CBO_FOR_DIM_CASE({n}, __VA_ARGS__)" for n in range(1, 8))
    assert macro == ("#define CBO_FOR_DIM(d, ...) switch (d) {" + cases +
                     " default: { constexpr int D = CBO_MAX_DIM; __VA_ARGS__; } break; }"), macro

    assert len(uses) >= 13, [u[0] for u in uses]
    for where, d, body in uses:
        assert d, where
        assert D_ARG.search(body), f"{where}: the body does not instantiate with D: {body.strip()}"
        assert not (TEMPLATE_ARG.search(body) or MACRO_ARG.search(body)), f"{where}: a literal instantiation: {body.strip()}"
