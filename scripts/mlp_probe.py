#!/usr/bin/env python3
"""Stage two's MLP probe measured: ``two_stage.MLPProbe`` (the training pass as one launch of one workgroup, the predictions and their
correct count as a second launch) and ``two_stage.evaluate_mlp`` end to end, against the same loop written with torch modules on the
same device in the same process — the reference's way (train_triplet.py:148-180): a fresh ``nn.Sequential`` moved to the device, per
training embedding one host-to-device copy of the row and of its label, forward, ``F.cross_entropy``, backward, ``Adam.step``,
``zero_grad``; per validation embedding a copy, a forward, an argmax and a ``.item()``.

    python scripts/mlp_probe.py                 every part, each in a child process under its own time limit; writes profiles/r08/mlp_probe.txt
    python scripts/mlp_probe.py synth E         1,051 / 117 synthetic rows of width E in this process
    python scripts/mlp_probe.py dd [N]          evaluate_mlp end to end on N DD-shaped graphs (default 1,168 = 1,051 / 117), GcnEncoderGraph
    python scripts/mlp_probe.py kernels         20 fit + predict launch pairs at E = 64 (to run under rocprofv3 --kernel-trace --stats:
                                                timeout -k 10 300 rocprofv3 --kernel-trace --stats -d OUT -- python scripts/mlp_probe.py kernels)

Times are host clocks around work that ends in a synchronise, median [min .. max] of REPS alternating windows; the kernel's time per
step is device events around FITS back-to-back fit launches over their steps."""
import os
import subprocess
import sys
import time

REPS, FITS, LIMIT_S = 5, 10, 420
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "r08", "mlp_probe.txt")


def main_all():
    parts = []
    for args in (["synth", "64"], ["synth", "384"], ["dd"]):
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        text = r.stdout.decode()
        print(text, end="")
        sys.stdout.flush()
        parts.append(text)
        if r.returncode != 0:                                # (a fault or a time-out: nothing more is started on the device)
            print("part %s ended with status %d: stopping" % (" ".join(args), r.returncode))
            sys.exit(r.returncode)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("scripts/mlp_probe.py on one MI355X\n\n" + "\n".join(parts))
    print("wrote", OUT)


def _setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _wall(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _fmt(v):
    import numpy as np
    return "%9.2f [%9.2f .. %9.2f] ms" % (float(np.median(v)), min(v), max(v))


def torch_loop(E_tr, y_tr, E_va, y_va, init):
    """the reference's loop on the device, from the six initial tensors ``init`` -> correct predictions (pred == label)"""
    import torch
    import torch.nn.functional as F
    from torch import nn
    layers = [nn.Linear(E_tr.shape[1], 64), nn.LeakyReLU(), nn.Linear(64, 32), nn.LeakyReLU(), nn.Linear(32, 2)]
    with torch.no_grad():
        for lin, w, b in zip(layers[0::2], init[0::2], init[1::2]):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    model = nn.Sequential(*[m.cuda() for m in layers])
    opt = torch.optim.Adam(model.parameters(), lr=0.001)
    for i in range(len(E_tr)):
        out = torch.unsqueeze(model(torch.from_numpy(E_tr[i]).cuda()), 0)
        loss = F.cross_entropy(out, torch.LongTensor([int(y_tr[i])]).cuda())
        loss.backward()
        opt.step()
        opt.zero_grad()
    correct = 0
    for i in range(len(E_va)):
        pred = model(torch.from_numpy(E_va[i]).cuda()).argmax(dim=0)
        correct += int(pred.item() == int(y_va[i]))
    return correct


def _initial(seed, E):
    import torch
    torch.manual_seed(seed)
    lins = [torch.nn.Linear(E, 64), torch.nn.Linear(64, 32), torch.nn.Linear(32, 2)]
    return [t.detach().clone() for m in lins for t in (m.weight, m.bias)]


def compare(tag, E_tr, y_tr, E_va, y_va):
    """both ways on the same embeddings (device tensors for the probe, host rows for the loop, as each takes them)"""
    import numpy as np
    import torch
    from two_stage_gnn_amd import _native as nat, two_stage as TS
    Eh_tr, Eh_va = E_tr.cpu().numpy(), E_va.cpu().numpy()
    y_tr, y_va = np.asarray(y_tr).astype(np.int64), np.asarray(y_va).astype(np.int64)
    assert set(np.unique(np.concatenate([y_tr, y_va])).tolist()) <= {0, 1}       # (the reference's last layer has two rows)
    n, nq, E = len(Eh_tr), len(Eh_va), Eh_tr.shape[1]
    init = _initial(0, E)

    def probe():
        p = TS.MLPProbe().fit(E_tr, y_tr, classes=np.array([0, 1]), init=init)
        return int(p.correct_count(E_va, y_va).cpu()), p

    def loop():
        return torch_loop(Eh_tr, y_tr, Eh_va, y_va, init)

    (_, (c_probe, p)), (_, c_loop) = _wall(probe), _wall(loop)                    # warm-up of both
    assert p.kernel_ok()
    times = {"probe": [], "loop": []}
    for _ in range(REPS):
        times["probe"].append(_wall(probe)[0])
        times["loop"].append(_wall(loop)[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cls = p.class_index(y_tr)
    losses = torch.empty(n, device="cuda")
    dims = p._dims()

    def launch():
        nat.call("mlp_probe_fit_f32", E_tr, E_tr.stride(0), cls, n, *dims, *p._params, p._exp_avg, p._exp_avg_sq, 0, p.lr, p.betas[0],
                 p.betas[1], p.eps, p.negative_slope, losses)
    launch()
    kernel = nat.last_kernel()
    e0.record()
    for _ in range(FITS):
        launch()
    e1.record()
    e1.synchronize()
    t_fit = e0.elapsed_time(e1) / FITS
    p.forward(E_va)
    e0.record()
    for _ in range(100):
        p.forward(E_va)
    e1.record()
    e1.synchronize()
    t_pred = e0.elapsed_time(e1) / 100
    print("%s: %d training rows, %d validation rows, width %d; median [min .. max] of %d alternating windows" % (tag, n, nq, E, REPS))
    print("  MLPProbe.fit + predict with count + its one copy          : %s" % _fmt(times["probe"]))
    print("  the loop with torch modules on the device (reference's way): %s" % _fmt(times["loop"]))
    print("  probe faster in every window: %s   (ratio of medians %.1fx)"
          % (all(a < b for a, b in zip(times["probe"], times["loop"])), np.median(times["loop"]) / np.median(times["probe"])))
    print("  fit launch alone (%s): %.3f ms = %.2f us per step; predict launch alone: %.1f us" % (kernel, t_fit, t_fit * 1e3 / n, t_pred * 1e3))
    print("  correct predictions: probe %d / %d, loop %d / %d" % (c_probe, nq, c_loop, nq))
    sys.stdout.flush()


def main_synth(E):
    import numpy as np
    import torch
    _setup()
    rng = np.random.default_rng(0)
    y, yq = rng.integers(0, 2, 1051), rng.integers(0, 2, 117)
    centre = 0.5 * rng.normal(size=(2, E))
    X = torch.from_numpy((centre[y] + rng.normal(size=(1051, E))).astype(np.float32)).cuda()
    Q = torch.from_numpy((centre[yq] + rng.normal(size=(117, E))).astype(np.float32)).cuda()
    compare("synthetic E = %d" % E, X, y, Q, yq)


def main_dd(n_graphs=1168):
    import numpy as np
    import torch
    _setup()
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import dense_encoders as Enc, two_stage as TS
    graphs, fin = dense_dataset(n_graphs)

    class A:
        bias = True
    torch.manual_seed(5)
    model = Enc.GcnEncoderGraph(fin, 128, 64, 2, 3, bn=True, args=A(), final_dim="output_dim").cuda()
    n_val = max(1, int(round(0.1 * n_graphs)))
    train, val = graphs[:n_graphs - n_val], graphs[n_graphs - n_val:]
    y_tr, y_va = TS._labels(train), TS._labels(val)
    init = _initial(0, 64)

    def end_to_end():
        return TS.evaluate_mlp(train, val, model, init=init)

    def reference_way():
        emb = TS.embed_dataset(model, train + val).cpu().numpy()               # (the embeddings the batched way; the probe the reference's)
        return {"acc": torch_loop(emb[:len(train)], y_tr, emb[len(train):], y_va, init) / len(val)}

    t_first, res = _wall(end_to_end)                                           # first evaluation: the graphs become resident
    _, res_ref = _wall(reference_way)
    times = {"hip": [], "ref": [], "embed": []}
    for _ in range(REPS):
        times["hip"].append(_wall(end_to_end)[0])
        times["ref"].append(_wall(reference_way)[0])
        times["embed"].append(_wall(lambda: TS.embed_dataset(model, train + val))[0])
    print("DD-shaped: %d graphs (%d train / %d validation), GcnEncoderGraph 3 layers h = 128, embedding width 64" % (n_graphs, len(train), len(val)))
    print("  two_stage.evaluate_mlp end to end                           : %s   (first call, graphs not yet resident: %.1f ms)"
          % (_fmt(times["hip"]), t_first))
    print("  embed_dataset + the loop with torch modules on the device   : %s" % _fmt(times["ref"]))
    print("  embed_dataset alone                                         : %s" % _fmt(times["embed"]))
    print("  accuracy: evaluate_mlp %.4f, torch loop %.4f" % (res["acc"], res_ref["acc"]))
    emb = TS.embed_dataset(model, train + val)
    compare("DD-shaped embeddings", emb[:len(train)], y_tr, emb[len(train):], y_va)


def main_kernels():
    import numpy as np
    import torch
    _setup()
    from two_stage_gnn_amd import two_stage as TS
    rng = np.random.default_rng(0)
    y = rng.integers(0, 2, 1051)
    X = torch.from_numpy((0.5 * rng.normal(size=(2, 64))[y] + rng.normal(size=(1051, 64))).astype(np.float32)).cuda()
    Q = torch.from_numpy(rng.normal(size=(117, 64)).astype(np.float32)).cuda()
    init = _initial(0, 64)
    for _ in range(20):
        TS.MLPProbe().fit(X, y, init=init).forward(Q)
    torch.cuda.synchronize()
    print("20 fit + predict launch pairs done")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "synth":
        main_synth(int(sys.argv[2]))
    elif len(sys.argv) >= 2 and sys.argv[1] == "dd":
        main_dd(int(sys.argv[2]) if len(sys.argv) > 2 else 1168)
    elif len(sys.argv) >= 2 and sys.argv[1] == "kernels":
        main_kernels()
    else:
        main_all()
