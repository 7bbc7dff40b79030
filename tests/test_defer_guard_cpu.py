"""The deferral guard of the layer nodes (pointwise._param_sinks_ok behind pointwise._bwd) on the host: both are plain Python over
the autograd graph, so every Function of factorizer_amd.pointwise is replaced by a stand-in with the SAME forward parameter
list, the same `_fz_acts` and the same decorators, whose backward returns zeros of the right shapes.  `_finish_scope` stays
off without a device tensor; what is checked is the decision alone.

`needs_input_grad` / `_fz_acts` count the arguments of `apply`, `ctx.next_functions` counts its tensor arguments only: with a
float eps in front of the weight (LNLinearFn) or a None bias in the middle (UpCatLinearFn with a bias-less transposed
convolution) the two differ.  Every case asserts that each parameter was judged by its OWN sink: `_Defer.seen` must hold the
id() of exactly the parameters passed."""
import inspect
import itertools

import pytest
import torch

from factorizer_amd import _native as N
from factorizer_amd import pointwise as PW

_FWD = getattr(PW, "_fwd", N.capture_products)   # the decorator of the real forwards

ACT, PARAM, BUF = "act", "param", "buf"   # a non-leaf activation | a leaf parameter | a tensor that needs no gradient
PRO = "pro"                               # the block prologue of the two producer nodes: a TUPLE (ln_w, ln_b, eps, w_in), no tensor


def _spec(**kw):
    return kw


# per Function: argument name -> kind | constant, and the arguments a real call site may pass as None (defaulted trailing
# arguments are also left out: _combos)
SPECS = {
    "LNLinearFn": (_spec(x=ACT, ln_w=PARAM, ln_b=PARAM, eps=1e-5, w=PARAM, b=PARAM, act="relu"), ("b",)),
    "ActLinearResFn": (_spec(z=ACT, w=PARAM, b=PARAM, res=ACT, bact="gelu"), ("b", "res")),
    "CatLinearFn": (_spec(x1=ACT, x2=ACT, w=PARAM, b=PARAM), ("b",)),
    "LinearFn": (_spec(x=ACT, w=PARAM, b=PARAM), ("b",)),
    "LayerNormFn": (_spec(x=ACT, w=PARAM, b=PARAM, eps=1e-5), ()),
    "ConvK2S2Fn": (_spec(x=ACT, w=PARAM, b=PARAM), ("b",)),
    "SkipConvK2S2Fn": (_spec(x=ACT, w=PARAM, b=PARAM), ("b",)),
    "TConvK2S2Fn": (_spec(x=ACT, w=PARAM, b=PARAM), ("b",)),
    "ConvK3Fn": (_spec(x=ACT, w=PARAM, b=PARAM, pro=PRO), ("b", "pro")),
    "UpCatLinearFn": (_spec(skip=ACT, deep=ACT, w_t=PARAM, b_t=PARAM, w_ad=PARAM, b_ad=PARAM, pro=PRO), ("b_t", "b_ad", "pro")),
    # the one-node block is only entered with in_proj bias-less and every other bias present (blocks.FactorizerBlock.forward),
    # and u0 / v0 are the buffers of a RandomInit (nmf.MatrixFactorization._native_solver refuses every other init): never None
    "FactorizerBlockFn": (_spec(x=ACT, n1w=PARAM, n1b=PARAM, win=PARAM, u0=BUF, v0=BUF, wout=PARAM, bout=PARAM, n2w=PARAM, n2b=PARAM,
                                w1=PARAM, b1=PARAM, w2=PARAM, b2=PARAM, cfg={"T": 5}, head_w=PARAM, head_b=PARAM, t_pre=ACT, st_pre=ACT),
                          ("head_w", "head_b", "t_pre", "st_pre")),
    "HeadOfBlockFn": (_spec(y=ACT, w=PARAM, b=PARAM, logits=ACT), ("b",)),
}


def _functions():
    return {n: c for n, c in vars(PW).items()
            if inspect.isclass(c) and issubclass(c, torch.autograd.Function) and c.__module__ == PW.__name__}


def _guarded(cls):
    """is cls.backward decorated with PW._bwd?"""
    return "_param_sinks_ok" in getattr(getattr(cls.backward, "__code__", None), "co_names", ())


def test_every_guarded_function_has_a_case():
    fns = _functions()
    guarded = {n for n, c in fns.items() if _guarded(c)}
    assert len(guarded) >= 12 and guarded == set(SPECS), (sorted(guarded - set(SPECS)), sorted(set(SPECS) - guarded))
    for n in guarded:
        spec, optional = SPECS[n]
        assert list(inspect.signature(fns[n].forward).parameters)[1:] == list(spec), n
        assert set(optional) <= set(spec), n
        if hasattr(PW, "_fwd"):   # a guarded backward needs the argument map of its forward
            assert "_fz_slots" in fns[n].forward.__code__.co_names, n


_STAND_INS = {}


def _stand_in(name, decorate_forward=True):
    """a Function with `name`'s forward parameter list, `_fz_acts` and decorators; its backward returns zeros"""
    key = (name, decorate_forward)
    if key in _STAND_INS:
        return _STAND_INS[key]
    real = _functions()[name]
    sig = inspect.signature(real.forward)

    def forward(ctx, *a):
        sig.bind(ctx, *a)   # (the real parameter list takes this call)
        ctx.shapes = [tuple(v.shape) if isinstance(v, torch.Tensor) else None for v in a]
        return a[0] * 1.0

    def backward(ctx, g):
        return tuple(torch.zeros(sh) if sh is not None and need else None for sh, need in zip(ctx.shapes, ctx.needs_input_grad))

    body = {"forward": staticmethod(_FWD(forward) if decorate_forward else N.capture_products(forward)),
            "backward": staticmethod(PW._bwd(backward))}
    if "_fz_acts" in vars(real):
        body["_fz_acts"] = real._fz_acts
    _STAND_INS[key] = type("StandIn" + name, (torch.autograd.Function,), body)
    return _STAND_INS[key]


def _arguments(name, absent=(), omit=()):
    """(args of apply, {argument name: leaf parameter}) with the arguments in `absent` passed as None, those in `omit` left out"""
    spec, _ = SPECS[name]
    acts = getattr(_functions()[name], "_fz_acts", (0,))
    args, params = [], {}
    for i, (k, kind) in enumerate(spec.items()):
        if k in omit:
            assert all(j in omit for j in list(spec)[i:]), "only a tail can be omitted"
            break
        if k in absent:
            v = None
        elif kind == ACT:
            v = torch.randn(2, 3, requires_grad=True) * 1
        elif kind == PARAM:
            v = torch.randn(3, i + 1, requires_grad=True)
            if i not in acts:   # (FactorizerBlockFn lists head_w / head_b as its activations: HeadOfBlockFn forms their gradients)
                params[k] = v
        elif kind == BUF:
            v = torch.randn(2, 2)
        elif kind == PRO:
            v = (torch.randn(3, requires_grad=True), torch.randn(3, requires_grad=True), 1e-5, torch.randn(3, 3, requires_grad=True))
        else:
            v = kind   # the real kind of constant: float eps, string act, dict cfg
        args.append(v)
    return args, params


def _armed_backward(build, owned, create_graph=False):
    """run `build()`'s scalar backward with deferral armed for `owned`; (refused nodes, seen ids)"""
    d = PW._Defer
    PW.defer_finishes(True)
    try:
        PW.arm_deferred_finishes(owned)
        assert d.armed
        r0 = d.refused
        build().sum().backward(create_graph=create_graph)
        return d.refused - r0, set(d.seen)
    finally:
        PW.defer_finishes(False)
        PW.arm_deferred_finishes(())


def _combos():
    for name, (spec, optional) in SPECS.items():
        for r in range(len(optional) + 1):
            for absent in itertools.combinations(optional, r):
                yield pytest.param(name, absent, (), id=f"{name}-none:{'+'.join(absent) or '-'}")
        tail = [k for k in reversed(list(spec)) if inspect.signature(_functions()[name].forward).parameters[k].default is not inspect.Parameter.empty]
        for n in range(1, len(tail) + 1):   # call sites that leave defaulted trailing arguments out (ConvK3Fn.apply(x, w, b))
            yield pytest.param(name, (), tuple(tail[:n]), id=f"{name}-omit:{'+'.join(tail[:n])}")


@pytest.mark.parametrize("name,absent,omit", list(_combos()))
def test_each_parameter_is_judged_by_its_own_sink(name, absent, omit):
    fn = _stand_in(name)
    args, params = _arguments(name, absent, omit)
    refused, seen = _armed_backward(lambda: fn.apply(*args), list(params.values()))
    assert refused == 0, (name, absent, omit)
    assert seen == {id(p) for p in params.values()}, (name, absent, omit, sorted(params))
    assert not PW._Defer.enabled and not PW._Defer.armed


NEG = [("LNLinearFn", (), "w"), ("LNLinearFn", ("b",), "w"), ("UpCatLinearFn", (), "w_ad"), ("UpCatLinearFn", ("b_t",), "w_ad"),
       ("UpCatLinearFn", ("b_t",), "b_ad")]


def _neg(case):
    name, absent, victim = case
    args, params = _arguments(name, absent)
    return _stand_in(name), args, params, list(SPECS[name][0]).index(victim), params[victim]


@pytest.mark.parametrize("case", NEG, ids=lambda c: f"{c[0]}-none:{'+'.join(c[1]) or '-'}-{c[2]}")
class TestRefusals:
    """one parameter of the node breaks one rule: the node runs its finishes at once (one `refused`), nothing raises"""

    def test_not_owned(self, case):
        fn, args, params, _, p = _neg(case)
        refused, seen = _armed_backward(lambda: fn.apply(*args), [q for q in params.values() if q is not p])
        assert refused == 1 and id(p) not in seen

    def test_grad_already_set(self, case):
        fn, args, params, _, p = _neg(case)
        p.grad = torch.zeros_like(p)
        assert _armed_backward(lambda: fn.apply(*args), list(params.values()))[0] == 1

    def test_tensor_hook(self, case):
        fn, args, params, _, p = _neg(case)
        p.register_hook(lambda g: g)
        assert _armed_backward(lambda: fn.apply(*args), list(params.values()))[0] == 1

    def test_post_accumulate_grad_hook(self, case):
        fn, args, params, _, p = _neg(case)
        got = []
        p.register_post_accumulate_grad_hook(lambda q: got.append(q.grad.clone()))
        assert _armed_backward(lambda: fn.apply(*args), list(params.values()))[0] == 1
        assert len(got) == 1 and torch.equal(got[0], p.grad)

    def test_owner_hook_keeps_deferring(self, case):
        """the hook the arming owner installed itself (FlatGradSync's bucket hook, registered through PW.owner_hook)"""
        fn, args, params, _, p = _neg(case)
        fired = []
        hook = PW.owner_hook(lambda q: fired.append(1))
        p.register_post_accumulate_grad_hook(hook)
        refused, seen = _armed_backward(lambda: fn.apply(*args), list(params.values()))
        assert refused == 0 and fired == [1] and seen == {id(q) for q in params.values()}
        p.register_post_accumulate_grad_hook(lambda q: None)   # ... and a stranger's next to it
        for q in params.values():
            q.grad = None
        again = [a.detach().requires_grad_(True) * 1 if isinstance(a, torch.Tensor) and a.grad_fn is not None else a for a in args]
        assert _armed_backward(lambda: fn.apply(*again), list(params.values()))[0] == 1

    def test_fed_through_a_computing_op(self, case):
        fn, args, params, i, p = _neg(case)
        args[i] = p * 1
        assert _armed_backward(lambda: fn.apply(*args), list(params.values()))[0] == 1

    def test_fed_through_a_view_defers(self, case):
        """(the counterpart: a reshape in front of the node is passed through, as the 1x1x1 weights of the modules are)"""
        fn, args, params, i, p = _neg(case)
        args[i] = p.view(p.shape)
        refused, seen = _armed_backward(lambda: fn.apply(*args), list(params.values()))
        assert refused == 0 and seen == {id(q) for q in params.values()}

    def test_used_by_two_nodes(self, case):
        fn, args, params, i, p = _neg(case)
        args2, params2 = _arguments(*case[:2])
        args2[i] = p   # the second node's other parameters are its own

        def build():
            y = fn.apply(*args)
            args2[0] = y
            return fn.apply(*args2)

        refused, seen = _armed_backward(build, list(params.values()) + list(params2.values()))
        assert refused == 1 and id(p) in seen   # the node that runs second in the backward is the one refused

    @pytest.mark.filterwarnings("ignore:Using backward.. with create_graph=True")
    def test_create_graph(self, case):
        fn, args, params, _, p = _neg(case)
        refused, seen = _armed_backward(lambda: fn.apply(*args), list(params.values()), create_graph=True)
        assert refused == 1 and not seen

    def test_no_argument_map(self, case):
        """a forward that recorded no argument map (or one that does not fit the node) refuses; it never raises"""
        if not hasattr(PW, "_fwd"):
            pytest.fail("pointwise._fwd is missing: the guard has no argument map to index next_functions with")
        name, absent, _ = case
        args, params = _arguments(name, absent)
        bare = _stand_in(name, decorate_forward=False)
        assert _armed_backward(lambda: bare.apply(*args), list(params.values()))[0] == 1

        class Lies(torch.autograd.Function):
            _fz_acts = getattr(_functions()[name], "_fz_acts", (0,))

            @staticmethod
            def forward(ctx, *a):
                ctx._fz_slots = tuple(range(len(a)))   # as if every argument were a tensor
                ctx.n = len(a)
                return a[0] * 1.0

            @staticmethod
            @PW._bwd
            def backward(ctx, g):
                return (g,) + (None,) * (ctx.n - 1)

        args, params = _arguments(name, absent)
        assert _armed_backward(lambda: Lies.apply(*args), list(params.values()))[0] == 1


def test_flat_grad_sync_registers_its_hooks_as_the_owners():
    """parallel.FlatGradSync installs post-accumulate-grad hooks when it overlaps collectives with the backward: they flush
    before they read, are registered through PW.owner_hook and must not cost the model its deferral"""
    from factorizer_amd import parallel

    lin = torch.nn.Linear(3, 2)
    sync = parallel.FlatGradSync.__new__(parallel.FlatGradSync)   # (the constructor's hook loop, without a process group)
    sync.buckets, sync._ready, sync._launched = [{"params": list(lin.parameters())}], [0], [False]
    launched = []
    sync._launch = launched.append
    hook = PW.owner_hook(sync._make_hook(0))
    for p in lin.parameters():
        p.register_post_accumulate_grad_hook(hook)
    fn = _stand_in("LinearFn")
    x = torch.randn(2, 3, requires_grad=True) * 1
    refused, seen = _armed_backward(lambda: fn.apply(x, lin.weight, lin.bias), list(lin.parameters()))
    assert refused == 0 and seen == {id(p) for p in lin.parameters()} and launched == [0]
    src = inspect.getsource(parallel.FlatGradSync.__init__)
    assert "owner_hook(" in src and "register_post_accumulate_grad_hook" in src
