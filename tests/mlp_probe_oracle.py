"""Oracle of the MLP-probe tests (test infrastructure; the product never imports it): the reference's evaluate_mlp() training loop
written with torch's own modules — ``nn.Linear`` / ``nn.LeakyReLU`` in an ``nn.Sequential``, ``F.cross_entropy`` on one row,
``optim.Adam.step`` per row — on the CPU, in float64 (THE reference: given the initial parameters the loop is deterministic) and in
float32 (how far an honest fp32 evaluation of the same loop lies from it: the yardstick of the tolerance).

Tolerance (every comparison of the code under test with the fp64 run): err(a) = max |a - fp64| over the whole array, and
err(code) <= max(10 err(cpu32), 1e-5 max(1, max |fp64|)).  Predictions: a query whose two largest fp64 logits differ by less than
2e-5 max(1, max |logit|) is undecided (each logit may move by the floor of the tolerance); undecided queries may be at most 2 % of a
case and every other prediction must be the fp64 one.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import knn_oracle as KO

CAP = 0.02
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


def initial(seed, E, hidden, C):
    """the reference's construction (three nn.Linear on the host, in order) after torch.manual_seed(seed) -> six float32 tensors"""
    torch.manual_seed(seed)
    lins = [torch.nn.Linear(E, hidden[0]), torch.nn.Linear(hidden[0], hidden[1]), torch.nn.Linear(hidden[1], C)]
    return [t.detach().clone() for m in lins for t in (m.weight, m.bias)]


def sequential(init, dtype, negative_slope=0.01):
    h1, E = init[0].shape
    h2, C = init[2].shape[0], init[4].shape[0]
    seq = torch.nn.Sequential(torch.nn.Linear(E, h1), torch.nn.LeakyReLU(negative_slope), torch.nn.Linear(h1, h2),
                              torch.nn.LeakyReLU(negative_slope), torch.nn.Linear(h2, C)).to(dtype)
    with torch.no_grad():
        for lin, w, b in zip((seq[0], seq[2], seq[4]), init[0::2], init[1::2]):
            lin.weight.copy_(w.to(dtype))
            lin.bias.copy_(b.to(dtype))
    return seq


def run(init, X, cls, Q, dtype, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, negative_slope=0.01):
    """the loop on the CPU in ``dtype`` -> {'losses' [n], 'logits' [nq, C], 'params': six arrays, 'exp_avg': Adam's first
    moments of the six}, float64 numpy"""
    model = sequential(init, dtype, negative_slope)
    opt = torch.optim.Adam(model.parameters(), lr=lr, betas=betas, eps=eps)
    Xt, Qt = torch.as_tensor(np.asarray(X)).to(dtype), torch.as_tensor(np.asarray(Q)).to(dtype)
    target = torch.as_tensor(np.asarray(cls)).long()
    losses = []
    for i in range(Xt.size(0)):
        out = torch.unsqueeze(model(Xt[i]), 0)
        loss = F.cross_entropy(out, target[i:i + 1])
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        logits = model(Qt) if Qt.size(0) else torch.zeros(0, init[4].shape[0])
    params = [p.detach().double().numpy().copy() for lin in (model[0], model[2], model[4]) for p in (lin.weight, lin.bias)]
    moments = [opt.state[p]["exp_avg"].double().numpy().copy() for lin in (model[0], model[2], model[4]) for p in (lin.weight, lin.bias)
               if "exp_avg" in opt.state[p]]
    return {"losses": np.asarray(losses, dtype=np.float64), "logits": logits.double().numpy(), "params": params, "exp_avg": moments}


@functools.lru_cache(maxsize=None)
def case(seed, n, q, D, C, hidden=(64, 32)):
    """data of ``knn_oracle.synthetic(seed, n, q, D, C, 0)``, initial parameters under torch.manual_seed(seed), and both CPU runs;
    computed once per process and shared (treat as read-only)"""
    X, y, Q, yq = KO.synthetic(seed, n, q, D, C, 0)
    init = initial(seed, D, hidden, C)
    return {"X": X, "y": y, "Q": Q, "yq": yq, "init": init, "f64": run(init, X, y, Q, torch.float64), "f32": run(init, X, y, Q, torch.float32)}


def bound(f64, f32):
    """the tolerance for one array: max(10 err(cpu32), 1e-5 max(1, max |fp64|))"""
    f64, f32 = np.asarray(f64, dtype=np.float64), np.asarray(f32, dtype=np.float64)
    e32 = float(np.abs(f32 - f64).max()) if f64.size else 0.0
    scale = max(1.0, float(np.abs(f64).max())) if f64.size else 1.0
    return max(10.0 * e32, 1e-5 * scale), e32


def check(tag, got, f64, f32):
    """prints the figures, then asserts err(got) <= bound"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.asarray(f64).shape, (tag, got.shape, np.asarray(f64).shape)
    b, e32 = bound(f64, f32)
    err = float(np.abs(got - f64).max()) if got.size else 0.0
    print("%s: err %.3g, err(cpu32) %.3g, bound %.3g" % (tag, err, e32, b))
    assert np.isfinite(got).all() and err <= b, (tag, err, b)
    return err


def check_run(tag, got, ref):
    """got: {'losses', 'logits', 'params'} of the code under test; ref: a ``case``"""
    check(tag + " losses", got["losses"], ref["f64"]["losses"], ref["f32"]["losses"])
    check(tag + " logits", got["logits"], ref["f64"]["logits"], ref["f32"]["logits"])
    for name, g, a, b in zip(NAMES, got["params"], ref["f64"]["params"], ref["f32"]["params"]):
        check(tag + " " + name, g, a, b)


def undecided(logits64):
    """bool [nq]: the two largest fp64 logits closer than 2e-5 max(1, max |logit|)"""
    l = np.asarray(logits64, dtype=np.float64)
    top = np.sort(l, axis=1)
    return (top[:, -1] - top[:, -2]) < 2e-5 * max(1.0, float(np.abs(l).max()))


def check_predictions(tag, pred_index, logits64):
    und = undecided(logits64)
    want = np.argmax(logits64, axis=1)
    top = np.sort(logits64, axis=1)
    print("%s: undecided %d / %d, smallest fp64 margin %.3g, predictions that differ %d"
          % (tag, und.sum(), und.size, (top[:, -1] - top[:, -2]).min(), (np.asarray(pred_index) != want).sum()))
    assert und.mean() <= CAP, (tag, und.sum(), und.size)
    assert ((np.asarray(pred_index) == want) | und).all(), tag
