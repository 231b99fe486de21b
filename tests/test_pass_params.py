"""Host side of the pass's hyper-parameters (channel ratio, softmax temperature, Gaussian scales): `PassParams`, the
hooks' three knobs, and the plumbing of tests/golden/pass_params_cases.json (make_pass_params_golden.py) -- its default
case and its ratio / temp cases reproduced by the CPU oracle's chain.  No GPU."""
import math
import pickle

import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import synth
from vidcom2_amd.models import _intercept as I
from vidcom2_amd.vidcom2 import PassParams, _c_params, _norm_params

from _stage_chain import canon_list, digest, oracle_chain
from conftest import load_json, make_input

CASES = load_json("pass_params_cases.json")["cases"]
REF_ALPHAS = [2 ** k for k in range(-3, 2)]
KNOBS = ("VC2_CHANNEL_RATIO", "VC2_TEMP", "VC2_ALPHAS")


def cid(c):
    extra = "".join(f"-{k}{c[k]:.4g}" for k in ("ratio", "temp") if c[k] is not None)
    if c["alphas"] is not None:
        extra += f"-a{len(c['alphas'])}"
    return f"{c['name']}-{c['F']}x{c['N']}x{c['D']}-{c['dtype']}-{c['dist']}{extra}"


# ---- PassParams ---------------------------------------------------------------------------------------------------
def test_exported():
    assert vc.PassParams is PassParams


def test_defaults_and_normalisation():
    p = PassParams()
    assert (p.channel_ratio, p.temp, p.alphas) == (0.5, 0.01, (0.125, 0.25, 0.5, 1.0, 2.0))
    assert p.is_default and _norm_params(p) is None and _norm_params(None) is None
    q = PassParams(0.5, 0.01, REF_ALPHAS)                 # the reference's own list (ints and floats)
    assert q == p and hash(q) == hash(p) and q.is_default and _norm_params(q) is None
    for other in (PassParams(0.25), PassParams(temp=0.05), PassParams(alphas=[1.0]),
                  PassParams(alphas=REF_ALPHAS[::-1])):   # (the order of the scales is part of the value)
        assert other != p and not other.is_default and _norm_params(other) is other
    with pytest.raises(TypeError):
        _norm_params((0.5, 0.01))


def test_immutable_hashable_picklable():
    p = PassParams(0.25, 0.05, [1, 2])
    assert p.alphas == (1.0, 2.0) and all(isinstance(a, float) for a in p.alphas)
    with pytest.raises(AttributeError):
        p.temp = 1.0
    with pytest.raises(AttributeError):
        del p.temp
    assert {p: 1}[PassParams(0.25, 0.05, (1.0, 2.0))] == 1
    assert len({PassParams(0.25), PassParams(0.25), PassParams(0.75)}) == 2
    assert pickle.loads(pickle.dumps(p)) == p
    assert "0.25" in repr(p) and "0.05" in repr(p)


@pytest.mark.parametrize("kw", [dict(alphas=[]), dict(alphas=[1.0, 0.0]), dict(alphas=[-1.0]),
                                dict(alphas=[float("nan")]), dict(alphas=[float("inf")]),
                                dict(temp=0.0), dict(temp=-0.01), dict(temp=float("inf")), dict(temp=float("nan")),
                                dict(channel_ratio=0.0), dict(channel_ratio=-0.5), dict(channel_ratio=1.0001),
                                dict(channel_ratio=float("nan")), dict(alphas=["x"])],
                         ids=lambda kw: next(iter(kw)) + "=" + str(next(iter(kw.values()))))
def test_validation(kw):
    with pytest.raises(ValueError):
        PassParams(**kw)


def test_alpha_count_limit():
    PassParams(alphas=[1.0] * 16)
    with pytest.raises(NotImplementedError):
        PassParams(alphas=[1.0] * 17)


@pytest.mark.parametrize("D", [64, 1001, 1024, 1536, 3584, 8192])
@pytest.mark.parametrize("ratio", [1 / 128, 0.25, 0.3, 0.5, 0.75, 1.0])
def test_channels_is_pythons_int(D, ratio):
    assert PassParams(ratio).channels(D) == int(D * ratio)


def test_channel_count_limits_on_the_host():
    with pytest.raises(ValueError):                       # int(64 / 128) == 0
        _c_params(PassParams(1 / 128), 64)
    with pytest.raises(NotImplementedError):              # 8192 channels scored
        _c_params(PassParams(1.0), 8192)
    assert _c_params(None, 8192) is None
    c = _c_params(PassParams(0.75, 0.5, [1, 2]), 3584)
    assert (c.channels, c.temp, c.n_alphas, list(c.alphas)[:3]) == (2688, 0.5, 2, [1.0, 2.0, 0.0])


def test_reference_signatures_unchanged():
    import inspect
    assert list(inspect.signature(vc.vidcom2_compression).parameters) == ["flattened_feat", "model", "base_scale",
                                                                          "frame_token_len", "img_feat"]
    assert list(inspect.signature(vc.select_low_var_channels).parameters) == ["x", "ratio"]
    assert list(inspect.signature(vc.compute_scales).parameters) == ["scores", "base", "temp"]
    assert list(inspect.signature(vc._multi_scale_gaussian).parameters) == ["x", "center", "alphas"]
    for fn in (vc.compress, vc.compress_batch, vc.vidcom2.CompressPlan.__init__):
        par = inspect.signature(fn).parameters
        assert list(par)[-1] == "params" and par["params"].default is None


# ---- the hooks' knobs ---------------------------------------------------------------------------------------------
@pytest.fixture
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_knobs_unset_is_no_params(knobs):
    assert I.pass_params() is None and I.params_kwargs() == {}


def test_knobs_parse(knobs):
    knobs.setenv("VC2_CHANNEL_RATIO", "0.25")
    assert I.pass_params() == PassParams(0.25)
    knobs.setenv("VC2_TEMP", "5e-2")
    knobs.setenv("VC2_ALPHAS", "0.1, 0.3,1,3")
    p = I.pass_params()
    assert p == PassParams(0.25, 0.05, [0.1, 0.3, 1.0, 3.0]) and I.params_kwargs() == {"params": p}
    knobs.delenv("VC2_CHANNEL_RATIO")
    knobs.delenv("VC2_TEMP")
    assert I.pass_params() == PassParams(alphas=[0.1, 0.3, 1.0, 3.0])
    knobs.setenv("VC2_ALPHAS", "0.125,0.25,0.5,1,2")       # the reference's own values: a PassParams that is the default
    assert I.pass_params().is_default


def test_knobs_are_read_at_call_time(knobs):
    assert I.pass_params() is None
    knobs.setenv("VC2_TEMP", "0.5")
    assert I.pass_params().temp == 0.5
    knobs.setenv("VC2_TEMP", "1.0")
    assert I.pass_params().temp == 1.0


@pytest.mark.parametrize("knob,value", [("VC2_CHANNEL_RATIO", "half"), ("VC2_CHANNEL_RATIO", "0"), ("VC2_CHANNEL_RATIO", "1.5"),
                                        ("VC2_CHANNEL_RATIO", ""), ("VC2_TEMP", "0"), ("VC2_TEMP", "-1"), ("VC2_TEMP", "cold"),
                                        ("VC2_TEMP", "inf"), ("VC2_ALPHAS", ""), ("VC2_ALPHAS", "1,,2"), ("VC2_ALPHAS", "1;2"),
                                        ("VC2_ALPHAS", "1,-2"), ("VC2_ALPHAS", "0")])
def test_malformed_knob_names_itself(knobs, knob, value):
    knobs.setenv(knob, value)
    with pytest.raises(ValueError, match=knob):
        I.pass_params()


def test_too_many_alphas_in_the_knob(knobs):
    knobs.setenv("VC2_ALPHAS", ",".join(["1"] * 17))
    with pytest.raises(NotImplementedError, match="VC2_ALPHAS"):
        I.pass_params()


def test_hooks_call_without_params_when_no_knob_is_set(knobs, monkeypatch):
    """The hooks' call into the pass with the knobs unset is the call they made before the knobs existed: the same
    positional and keyword arguments, no `params`."""
    import vidcom2_amd.models.llava_hf as HF
    import vidcom2_amd.models.qwen2_5_vl as HQ
    import vidcom2_amd.models.qwen2_vl as HQ2
    seen = []

    class Res:
        global_idx = torch.arange(3)

    def fake(*a, **k):
        seen.append((a[1:], k))
        return Res()

    def fake_batch(clips, *a, **k):
        seen.append((a, k))
        return [Res() for _ in clips]

    for mod in (HQ, HQ2, HF):
        monkeypatch.setattr(mod, "compress", fake)
    for mod in (HQ, HF):
        monkeypatch.setattr(mod, "compress_batch", fake_batch)
    x = torch.zeros(8 * 16, 32)
    grid = torch.tensor([8, 8, 8])
    HQ._compute_keep_indices(x, grid, 2, 0.25)
    HQ._compute_keep_indices_many([x], grid[None], 2, 0.25)
    HQ2._keep_index(x, grid[None], 2)
    HF._keep_indices(x, 16, 0.25)
    HF._keep_indices_many([x], 16, 0.25)
    assert seen == [((16, 0.25, "linear"), dict(gather=False)), (([16], 0.25), dict(gather=False)),
                    ((16, 0.25, "linear"), dict(gather=False)), ((16, 0.25, "linear"), dict(gather=False, stats_ws=None)),
                    ((16, 0.25), dict(gather=False))]
    del seen[:]
    knobs.setenv("VC2_TEMP", "0.5")
    p = PassParams(temp=0.5)
    HQ._compute_keep_indices(x, grid, 2, 0.25)
    HQ._compute_keep_indices_many([x], grid[None], 2, 0.25)
    HQ2._keep_index(x, grid[None], 2)
    HF._keep_indices(x, 16, 0.25)
    HF._keep_indices_many([x], 16, 0.25)
    assert [k["params"] for _, k in seen] == [p] * 5


# ---- the fixture's plumbing -----------------------------------------------------------------------------------------
def test_fixture_covers_what_it_must():
    assert sum(1 for c in CASES if c["ratio"] is None and c["temp"] is None and c["alphas"] is None) == 1
    al = [c["alphas"] for c in CASES if c["alphas"] is not None]
    assert [1.0] in al and [1, 2] in al and [0.5, 0.5] in al and [0.1, 0.3, 1.0, 3.0] in al
    assert [2.0 ** k for k in range(-5, 3)] in al and any(len(a) == 16 for a in al)
    assert any(isinstance(a, int) for c in CASES if c["alphas"] for a in c["alphas"])      # Python ints survive the JSON
    assert {c["dtype"] for c in CASES} == {"bf16", "f16", "f32"} and {c["dist"] for c in CASES} == {"drift", "cancel", "iid"}
    assert {c["D"] for c in CASES} == {1024, 1536, 3584}
    assert all(6 <= c["F"] <= 16 and 100 <= c["N"] <= 324 for c in CASES)
    assert any(c["ratio"] is not None and c["temp"] is not None and c["alphas"] is not None for c in CASES)
    vid = [c for c in CASES if c["model"] == "llava_vid"]
    assert len(vid) == 1 and vid[0]["N"] == 169 and "gidx_sha256" in vid[0]
    for c in CASES:
        if c["dtype"] == "f32":
            assert c["margin_gap"] > 1e-5 and c["margin_half"] > c["N"] * 1e-5
        PassParams(0.5 if c["ratio"] is None else c["ratio"], 0.01 if c["temp"] is None else c["temp"],
                   REF_ALPHAS if c["alphas"] is None else c["alphas"])


@pytest.mark.parametrize("c", [c for c in CASES if c["alphas"] is None and c["dtype"] != "f32"], ids=cid)
def test_oracle_chain_reproduces_the_ratio_and_temp_cases(c):
    """Generator plumbing: seeds, the rebinding of the reference's defaults and the stored digests, against the CPU
    oracle in `torch` mode (which has ratio and temp, not the alphas)."""
    assert c["oracle"]["torch"] == dict(sel=True, ks=True, keep=True, v=True, f=True, s=True, total=True, scales=True)
    x = make_input(c["F"], c["N"], c["D"], c["dtype"], c["seed"], c["dist"])
    assert synth.sha256_tensor(x) == c["x_sha256"], "synthetic generator is not bit-portable"
    O.set_mode("torch")
    o = oracle_chain(x, c["N"], c["base"], c["ratio"], c["temp"])
    assert o["sel"].shape[1] == int(c["D"] * (0.5 if c["ratio"] is None else c["ratio"]))
    assert digest(o["v"]) == c["v_sha256"] and digest(o["f"]) == c["f_sha256"]
    assert canon_list(o["s"]) == c["s"] and canon_list(o["scales"]) == c["scales"]
    assert o["ks"] == c["ks"] and int(o["keep"].numel()) == c["K"] and digest(o["keep"]) == c["keep_sha256"]
    assert digest(x[o["keep"]]) == c["rows_sha256"]
    assert all(math.isfinite(v) for v in c["s"])
