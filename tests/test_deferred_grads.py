"""GPU: how the gradients of the bucketed autograd models arrive when their weight-gradient sums are deferred to the end of the
backward pass (models/flat_buckets.py:grad_slot, _native.defer_begin / defer_reset).  MobileNetV3Wakeword, GRUWakeword,
CRNNWakeword and LSTMWakeword, each compared per tensor with a plain ``backward()`` of the same inputs (dropout 0: every
training pass of the same batch computes the same gradients):

1. two backward passes without zero_grad accumulate exactly g + g;
2. a tensor hook on a parameter sees the final gradient, not the partial values of a deferred sum;
3. ``backward(create_graph=True)`` leaves the right ``.grad``, and the fused optimizer step after it (through gather_grads)
   moves the parameters as after a plain backward;
4. ``torch.autograd.grad`` returns the right tensors, which a later backward leaves alone (they must not alias the bucket);
5. two instances, each under ``torch.utils.checkpoint(use_reentrant=False)``, summed: both get their gradients (the recompute
   forward runs inside the backward pass and must not discard the sums the other instance queued).

Where both sides run the same kernels the gradients must agree bit for bit: the recurrent models in every case (their
immediate and deferred partial sums are the same arithmetic) and MobileNetV3 where both sides defer.  MobileNetV3's split-K
weight gradients summed immediately (k_splitk_sum: an fp32 loop) and deferred (k_reduce_items: double) differ by round-off,
so where one side does not defer -- a second pass accumulating, a hooked parameter, create_graph, autograd.grad -- its
tensors are compared within 1e-6 of the tensor's largest entry: a sum that was not run leaves values of order one off.
Every test prints how many tensors agree bit for bit."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = ["mobilenetv3", "gru", "crnn", "lstm"]
TOL = 1e-6


def _make(name, seed=3):
    torch.manual_seed(seed)
    if name == "mobilenetv3":
        from wakeword_trainer_home_amd.models.mobilenet import MobileNetV3Wakeword
        m, shape = MobileNetV3Wakeword(dropout=0.0), (8, 1, 40, 151)
    elif name == "gru":
        from wakeword_trainer_home_amd.models.recurrent import GRUWakeword
        m, shape = GRUWakeword(input_size=40, dropout=0.0), (8, 1, 40, 101)
    elif name == "crnn":
        from wakeword_trainer_home_amd.models.recurrent import CRNNWakeword
        m, shape = CRNNWakeword(dropout=0.0), (8, 1, 40, 101)
    else:
        from wakeword_trainer_home_amd.models.lstm import LSTMWakeword
        m, shape = LSTMWakeword(input_size=40, dropout=0.0), (8, 1, 40, 101)
    m = m.to(DEV).train()
    with torch.no_grad():
        for mod in m.modules():                     # non-trivial BatchNorm affine parameters (MobileNetV3, CRNN front-end)
            if hasattr(mod, "running_mean") and isinstance(getattr(mod, "weight", None), torch.nn.Parameter):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.2)
    _ = m.flat_grad                                 # the bucket and its slots, as the optimizer / Trainer build them
    g = torch.Generator().manual_seed(seed + 10)
    x = (torch.randn(*shape, generator=g) * 2 - 4).to(DEV)
    w = torch.randn(shape[0], 2, generator=g).to(DEV)
    return m, x, w


def _loss(m, x, w):
    return (m(x) * w).sum()


def _plain(m, x, w):
    m.zero_grad(set_to_none=True)
    _loss(m, x, w).backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / max(ref.double().abs().max().item(), 1e-30)


def _check(tag, got, ref, exact):
    """got / ref: dicts by parameter name.  exact: every tensor bit for bit; else within TOL of its reference."""
    assert set(got) == set(ref), tag
    errs = {n: _rel(got[n], ref[n]) for n in ref}
    same = sum(torch.equal(got[n], ref[n]) for n in ref)
    worst = max(errs, key=errs.get)
    print(f"\n{tag}: {same}/{len(ref)} bit-exact, worst {worst} {errs[worst]:.2e}")
    bad = {n: e for n, e in errs.items() if not (torch.equal(got[n], ref[n]) if exact else e <= TOL)}
    assert not bad, f"{tag}: {bad}"


@pytest.mark.parametrize("name", MODELS)
def test_plain_backward_adopts_the_bucket_slots(name):
    """The default path is unchanged: a plain backward leaves the deferring models' gradients in their bucket slots."""
    m, x, w = _make(name)
    _plain(m, x, w)
    born = [p.grad.data_ptr() == v.data_ptr() for p, v in zip(m._fb_plist, m._fb_views)]
    if name == "mobilenetv3":
        assert all(born)
    else:
        assert sum(born) >= 8                       # the recurrent layers' weights and biases
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


@pytest.mark.parametrize("name", MODELS)
def test_two_backward_passes_accumulate(name):
    m, x, w = _make(name)
    ref = _plain(m, x, w)
    m.zero_grad(set_to_none=True)
    _loss(m, x, w).backward()
    _loss(m, x, w).backward()
    torch.cuda.synchronize()
    _check(f"{name} accumulate", {n: p.grad for n, p in m.named_parameters()}, {n: 2 * g for n, g in ref.items()},
           name != "mobilenetv3")


def _flowing(name, m):
    """The parameters whose gradients flow through autograd: all but CRNNWakeword's conv front-end, which adds its gradients to
    .grad itself (ww_cnn_front_bwd), so that its tensor hooks and torch.autograd.grad never see them, deferred or not."""
    return [(n, p) for n, p in m.named_parameters() if not (name == "crnn" and n.startswith("front."))]


@pytest.mark.parametrize("name", MODELS)
def test_tensor_hooks_see_the_final_gradient(name):
    m, x, w = _make(name)
    ref = _plain(m, x, w)
    m.zero_grad(set_to_none=True)
    seen, handles = {}, []
    named = list(m.named_parameters())
    for n, p in _flowing(name, m)[::3]:                         # every third tensor: hooked and unhooked ones in the same pass
        handles.append(p.register_hook(lambda g, n=n: seen.__setitem__(n, g.clone())))
    _loss(m, x, w).backward()
    torch.cuda.synchronize()
    for h in handles:
        h.remove()
    assert set(seen) == {n for n, _ in _flowing(name, m)[::3]}
    _check(f"{name} hook", seen, {n: ref[n] for n in seen}, name != "mobilenetv3")
    _check(f"{name} hook .grad", {n: p.grad for n, p in named}, ref, name != "mobilenetv3")


@pytest.mark.parametrize("name", MODELS)
def test_create_graph_backward_then_fused_step(name):
    from wakeword_trainer_home_amd.training.optimizer_factory import FlatFusedOptimizer
    m, x, w = _make(name)
    twin = copy.deepcopy(m)
    _ = twin.flat_grad
    ref = _plain(m, x, w)
    twin.zero_grad(set_to_none=True)
    _loss(twin, x, w).backward(create_graph=True)
    torch.cuda.synchronize()
    _check(f"{name} create_graph", {n: p.grad.detach() for n, p in twin.named_parameters()}, ref, name != "mobilenetv3")
    for n, p in twin.named_parameters():            # (break the parameter <-> gradient reference cycle create_graph makes)
        p.grad = p.grad.detach()
    steps = []
    for model in (m, twin):
        opt = FlatFusedOptimizer(model, "adamw", lr=1e-2, weight_decay=1e-2)
        opt.step()
        torch.cuda.synchronize()
        steps.append({n: p.detach().clone() for n, p in model.named_parameters()})
    _check(f"{name} step after create_graph", steps[1], steps[0], name != "mobilenetv3")


@pytest.mark.parametrize("name", MODELS)
def test_autograd_grad_returns_its_own_tensors(name):
    m, x, w = _make(name)
    ref = _plain(m, x, w)
    m.zero_grad(set_to_none=True)
    names, params = zip(*_flowing(name, m))
    got = torch.autograd.grad(_loss(m, x, w), params)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in params)
    kept = [g.clone() for g in got]
    _check(f"{name} autograd.grad", dict(zip(names, got)), {n: ref[n] for n in names}, name != "mobilenetv3")
    x2 = torch.flip(x, dims=[0]) * 0.5              # a later backward of another batch
    _loss(m, x2, w).backward()
    torch.cuda.synchronize()
    changed = [n for n, a, b in zip(names, got, kept) if not torch.equal(a, b)]
    assert not changed, f"{name}: a later backward changed the returned gradients {changed[:5]}"


@pytest.mark.parametrize("name", MODELS)
def test_two_checkpointed_instances(name):
    from torch.utils.checkpoint import checkpoint
    m1, x, w = _make(name, seed=3)
    m2, _, _ = _make(name, seed=4)
    for m in (m1, m2):
        m.zero_grad(set_to_none=True)
    (_loss(m1, x, w) + _loss(m2, x, w)).backward()
    torch.cuda.synchronize()
    ref = [{n: p.grad.clone() for n, p in m.named_parameters()} for m in (m1, m2)]
    for m in (m1, m2):
        m.zero_grad(set_to_none=True)
    out = checkpoint(m1, x, use_reentrant=False) + checkpoint(m2, x, use_reentrant=False)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    for i, m in enumerate((m1, m2)):
        _check(f"{name} checkpoint instance {i}", {n: p.grad for n, p in m.named_parameters()}, ref[i], True)
