"""A two-rank ``TrainEncoder`` training step held to a one-process reference, bit for bit (infrastructure: no tests here;
``test_dist_step_cpu.py`` and ``test_gpu_dist_step.py`` use it).

Three parts.

* **The step**, shared by the ranks and the reference: ``build`` makes the encoder from a seed, ``data`` makes fresh images
  from (seed, rank, step) -- fresh every step, so that a gradient read from a stale static buffer shows --, ``loss_of``
  weights every output of every frame with fixed random cotangents (every head gets a gradient), Adam is the optimiser.
* **The rank program** (``python -m torch.distributed.run --nproc-per-node 2 tests/dist_step.py --cfg ... --out DIR``): gloo,
  every rank on the one device; ``GradBucketer`` takes the gradients ``TrainEncoder`` hands over.  After every step a rank
  saves one file: the gradients after ``finish()`` (``None`` kept), the parameters and buffers after ``opt.step()``.
* **The reference** (``reference``), one process, no process group: one encoder copy PER RANK with the same initial
  parameters and ITS OWN BatchNorm buffers -- the project does not synchronise buffers between ranks (``GradBucketer`` only
  sees parameters; running statistics stay each rank's own), so they must differ between ranks and equal the copy's.  Each
  copy is a ``TrainEncoder(graphs=False)``
  and takes its rank's data; the mean follows ``GradBucketer``'s stated contract: ``None`` on every rank stays ``None``,
  ``None`` on some ranks counts as zeros, otherwise ``(g0 + g1) / 2`` in fp32 (gloo: one addition, which does not depend on
  the order, and one ``div_(2)``).  The mean is written into both copies and each takes an Adam step.

What this holds and what it does not.  The kernels behind the gradients are held to fp64 references elsewhere
(``test_gpu_train_encoder*.py``, ``test_gpu_deterministic.py``); here they are only required to be THE SAME FUNCTION on both
sides: in the deterministic mode a ``TrainEncoder`` step gives the same bits eagerly, in graph replay and across processes,
so the gradients and parameters of the two-rank run are a function of the inputs one process can compute, and the
comparison needs no tolerance.  What is under test is everything between the kernels and the optimiser: the hub leaves that
sum the plans in flight, the one-segment-late hand-over, ``_deliver``, the bucketer's packing from static graph buffers, the
collectives' pairing, the used-mask, the re-pointing of ``p.grad``.

``compare(got, ref)`` -> {(step, rank, kind): names that differ}, kind in ``KINDS``.
"""
import argparse
import contextlib
import json
import os
import signal
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KINDS = ("gradient", "none_pattern", "parameter", "buffer")
WORLD = 2

# The CPU trial's step: ResNet-34 with 32-channel heads in fp32, two frames of 1 x 3 x 32 x 48, one backward, one thread.
# 21.8 M parameters = 87 MB of fp32 gradients: bucket_mb = 25 gives four buckets.
CPU_CFG = dict(arch="resnet34", hidden=32, dtype="float32", device="cpu", shape=(1, 3, 32, 48), frames=2, steps=3,
               bucket_mb=25.0, overlap=True, set_to_none=True, graphs=False, overlap_wgrad=True, deterministic=None,
               det_conv="library", skip_refine=None, seed=31, lr=1e-3, threads=1)


def config(base=None, **kw):
    cfg = dict(CPU_CFG if base is None else base)
    unknown = set(kw) - set(cfg)
    assert not unknown, unknown
    cfg.update(kw)
    cfg["shape"] = tuple(cfg["shape"])
    if cfg["skip_refine"] is not None:
        cfg["skip_refine"] = tuple(cfg["skip_refine"])              # (rank, step): that rank leaves refine_input_feat out
    return cfg


# ---- the step, shared by the ranks and the reference -------------------------------------------------------------------
@contextlib.contextmanager
def mode(cfg):
    """The process settings of a run: thread count, the deterministic mode (True: the project's setting on and the library
    flags as the reference's trainer sets them; False: off; None: untouched) and its convolution route.  Restored on exit."""
    import dmm_net_amd
    from dmm_net_amd.determinism import get_deterministic_conv, get_deterministic_setting
    old = (torch.get_num_threads(), get_deterministic_setting(), get_deterministic_conv(),
           torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    try:
        if cfg["threads"]:
            torch.set_num_threads(int(cfg["threads"]))
        if cfg["deterministic"] is not None:
            det = bool(cfg["deterministic"])
            dmm_net_amd.set_deterministic(det)
            torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det, False
        dmm_net_amd.set_deterministic_conv(cfg["det_conv"])
        yield
    finally:
        torch.set_num_threads(old[0])
        dmm_net_amd.set_deterministic(old[1])
        dmm_net_amd.set_deterministic_conv(old[2])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old[3], old[4]


def build(cfg, graphs=None):
    """-> (FeatureEncoder, TrainEncoder over it): the same parameters and buffers wherever it is called with the same seed."""
    from dmm_net_amd.encoder import FeatureEncoder
    from dmm_net_amd.train_encoder import TrainEncoder
    torch.manual_seed(cfg["seed"])
    enc = FeatureEncoder(cfg["arch"], hidden_size=cfg["hidden"]).to(cfg["device"]).train()
    te = TrainEncoder(enc, dtype=getattr(torch, cfg["dtype"]), graphs=cfg["graphs"] if graphs is None else graphs,
                      overlap_wgrad=cfg["overlap_wgrad"])
    return enc, te


def data(cfg, rank, step):
    """The frames of one clip for ``rank`` at ``step``: seeded per rank AND per step (made on the host, so the same bits
    reach every device)."""
    g = torch.Generator().manual_seed(1_000_003 * cfg["seed"] + 7919 * rank + step)
    return [torch.randn(cfg["shape"], generator=g).to(cfg["device"]) for _ in range(cfg["frames"])]


def _outputs(out):
    return list(out["backbone_feature"]), list(out["refine_input_feat"])


def loss_of(cfg, outs, cots, skip_refine=False):
    """sum over frames and outputs of <output, cotangent>; the cotangents are fixed random tensors made once per (frame,
    output) from the seed (``cots``: the cache, filled at the first call).  ``skip_refine``: leave the ``refine_input_feat``
    outputs out (their heads then receive no gradient from this rank)."""
    total = None
    for f, out in enumerate(outs):
        prop, refine = _outputs(out)
        for k, o in enumerate(prop + ([] if skip_refine else refine)):
            key = (f, k)
            if key not in cots:
                g = torch.Generator().manual_seed(2_000_003 * cfg["seed"] + 101 * f + k)
                cots[key] = torch.randn(tuple(o.shape), generator=g).to(o.device)
            term = (o.float() * cots[key]).sum()
            total = term if total is None else total + term
    return total


def forward_backward(cfg, te, rank, step, cots):
    skip = cfg["skip_refine"] is not None and tuple(cfg["skip_refine"]) == (rank, step)
    outs = [te(img) for img in data(cfg, rank, step)]                 # one plan per frame in flight, ONE backward
    loss = loss_of(cfg, outs, cots, skip)
    loss.backward()
    return float(loss.detach())


def optimizer(cfg, enc):
    return torch.optim.Adam(enc.parameters(), lr=cfg["lr"])


def _cpu(t):
    return None if t is None else t.detach().to("cpu", copy=True)


def _save_step(outdir, rank, step, grads, enc, loss):
    rec = {"grads": grads, "params": {n: _cpu(p) for n, p in enc.named_parameters()},
           "buffers": {n: _cpu(b) for n, b in enc.named_buffers()}, "loss": loss}
    tmp = os.path.join(outdir, f"r{rank}_s{step}.tmp")
    torch.save(rec, tmp)
    os.replace(tmp, os.path.join(outdir, f"r{rank}_s{step}.pt"))


class Saved:
    """The files of a run: ``saved[step][rank]`` -> {"grads", "params", "buffers", "loss"}, read when asked for (a step of a
    ResNet-34 is 170 MB per rank; nothing is kept)."""

    def __init__(self, outdir, steps, world=WORLD):
        self.outdir, self.steps, self.world = outdir, steps, world

    def __getitem__(self, step):
        assert 0 <= step < self.steps
        return [torch.load(os.path.join(self.outdir, f"r{r}_s{step}.pt"), map_location="cpu") for r in range(self.world)]

    def meta(self, rank):
        with open(os.path.join(self.outdir, f"r{rank}_meta.json")) as f:
            return json.load(f)


# ---- the rank program --------------------------------------------------------------------------------------------------
def rank_main(cfg, outdir):
    import torch.distributed as dist
    from dmm_net_amd.distributed import GradBucketer, init_from_env
    t0 = time.time()
    if cfg["device"] != "cpu":
        torch.cuda.set_device(torch.device(cfg["device"]))
    rank, world = init_from_env("gloo")
    assert world == WORLD, world
    with mode(cfg):
        enc, te = build(cfg)
        opt = optimizer(cfg, enc)
        gb = GradBucketer(list(enc.parameters()), bucket_mb=cfg["bucket_mb"], overlap=cfg["overlap"])
        cots, losses = {}, []
        for step in range(cfg["steps"]):
            opt.zero_grad(set_to_none=cfg["set_to_none"])
            loss = forward_backward(cfg, te, rank, step, cots)
            gb.finish() if cfg["overlap"] else gb.all_reduce_mean()
            grads = {n: _cpu(p.grad) for n, p in enc.named_parameters()}
            opt.step()
            if cfg["device"] != "cpu":
                torch.cuda.synchronize()
            _save_step(outdir, rank, step, grads, enc, loss)
            losses.append(loss)
        gb.remove_hooks()
        meta = {"buckets": gb.num_collectives(), "launch_log": gb.launch_log, "host_syncs": gb.host_syncs, "losses": losses,
                "plans": sum(len(v) for v in te._plans.values()), "wall_s": time.time() - t0}
    dist.barrier()
    dist.destroy_process_group()
    with open(os.path.join(outdir, f"r{rank}_meta.json"), "w") as f:
        json.dump(meta, f)


class ChildFailed(RuntimeError):
    """The two-rank child ended badly; ``abnormal``: by a signal or at its time limit (nothing more may start after it)."""

    def __init__(self, msg, abnormal):
        super().__init__(msg)
        self.abnormal = abnormal


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(cfg, outdir, limit_s, env=None):
    """The rank program of this file for ``cfg``.  -> (``Saved``, wall seconds)."""
    wall = launch([os.path.abspath(__file__), "--cfg", json.dumps(cfg), "--out", outdir], outdir, limit_s, env)
    return Saved(outdir, cfg["steps"]), wall


def launch(program, outdir, limit_s, env=None):
    """``program`` (a script and its arguments) as two fresh rank processes under ``torch.distributed.run``, in a process group
    of their own and under ONE time limit: at the limit the launcher and both ranks are killed together.  -> wall seconds."""
    os.makedirs(outdir, exist_ok=True)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(WORLD), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port())] + list(program)
    log = os.path.join(outdir, "ranks.log")
    t0 = time.time()
    with open(log, "w") as lf:
        p = subprocess.Popen(cmd, cwd=ROOT, env=dict(os.environ, **(env or {})), stdout=lf, stderr=subprocess.STDOUT,
                             start_new_session=True)
        try:
            rc = p.wait(timeout=limit_s)
        except subprocess.TimeoutExpired:
            rc = None
        finally:
            try:
                os.killpg(p.pid, signal.SIGKILL)                      # (whatever is left of the group, the ranks included)
            except (ProcessLookupError, PermissionError):
                pass
            p.wait()
    wall = time.time() - t0
    if rc != 0:
        with open(log, errors="replace") as lf:
            tail = lf.read()[-4000:]
        if rc is None:
            raise ChildFailed(f"the two-rank run did not end within {limit_s} s and was killed\n{tail}", True)
        abnormal = rc < 0 or any(s in tail for s in ("Signal ", "SIGABRT", "SIGSEGV", "exitcode  : -", "illegal memory access"))
        raise ChildFailed(f"the two-rank run ended with exit code {rc}\n{tail}", abnormal)
    return wall


# ---- the reference -----------------------------------------------------------------------------------------------------
def segment_param_names(cfg, segment):
    """The names (as ``FeatureEncoder.named_parameters`` gives them) of the parameters ``TrainEncoder`` hands over with
    ``segment``."""
    enc, te = build(dict(cfg, device="cpu"), graphs=False)
    names = {id(p): n for n, p in enc.named_parameters()}
    return sorted(names[id(p)] for p in te._seg_params()[segment])


def mean_of(local):
    """``GradBucketer``'s contract for one parameter, ``local`` = its gradient on every rank: None everywhere -> None, None
    somewhere -> zeros there, then (g0 + g1) / 2 in fp32."""
    if all(g is None for g in local):
        return None
    some = next(g for g in local if g is not None)
    terms = [torch.zeros_like(some) if g is None else g for g in local]
    total = terms[0].clone()
    for t in terms[1:]:
        total += t
    return total.div_(len(local))


def reference(cfg, outdir, stale_segment=None, same_data=False):
    """The two-rank run of ``cfg`` computed in THIS process without a process group (module docstring).  Writes the same files
    as the ranks into ``outdir``.  -> ``Saved``.

    Two options make a WRONG reference on purpose, for the tests that show ``compare`` bites: ``stale_segment``: from step 1
    on, every rank's local gradients of that segment's parameters are the PREVIOUS step's (what a read of a static buffer
    that was not refreshed would deliver); ``same_data``: both ranks take rank 0's data."""
    os.makedirs(outdir, exist_ok=True)
    with mode(cfg):
        copies = [build(cfg, graphs=False) for _ in range(WORLD)]
        for enc, _ in copies[1:]:
            assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), copies[0][0].state_dict().values()))
        opts = [optimizer(cfg, enc) for enc, _ in copies]
        cots = [{} for _ in copies]
        stale = set(segment_param_names(cfg, stale_segment)) if stale_segment else set()
        prev = [None] * WORLD
        persistent = set()                     # zero_grad(set_to_none=False): a gradient that existed once stays a tensor
        for step in range(cfg["steps"]):
            local, losses = [], []
            for r, ((enc, te), opt) in enumerate(zip(copies, opts)):
                opt.zero_grad(set_to_none=True)
                losses.append(forward_backward(cfg, te, 0 if same_data else r, step, cots[r]))
                g = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in enc.named_parameters()}
                if stale and prev[r] is not None:
                    used, prev[r] = dict(g, **{n: prev[r][n] for n in stale}), g
                    g = used
                else:
                    prev[r] = g
                local.append(g)
            mean = {}
            for n in local[0]:
                m = mean_of([g[n] for g in local])
                if m is None and n in persistent:
                    m = torch.zeros_like(dict(copies[0][0].named_parameters())[n])
                mean[n] = m
            if not cfg["set_to_none"]:
                persistent |= {n for n, m in mean.items() if m is not None}
            for r, ((enc, te), opt) in enumerate(zip(copies, opts)):
                for n, p in enc.named_parameters():
                    p.grad = None if mean[n] is None else mean[n].clone()
                opt.step()
                if cfg["device"] != "cpu":
                    torch.cuda.synchronize()
                _save_step(outdir, r, step, {n: _cpu(m) for n, m in mean.items()}, enc, losses[r])
                opt.zero_grad(set_to_none=True)
    return Saved(outdir, cfg["steps"])


# ---- the comparer --------------------------------------------------------------------------------------------------------
def _differ(a, b):
    return sorted(n for n in a.keys() | b.keys()
                  if n not in a or n not in b or a[n].shape != b[n].shape or not torch.equal(a[n], b[n]))


def compare(got, ref):
    """-> {(step, rank, kind): the names that differ}, only the entries that have any.  ``gradient``: both sides have a tensor
    and the bits differ; ``none_pattern``: one side has ``None`` where the other has a tensor."""
    out = {}
    assert got.steps == ref.steps and got.world == ref.world
    for step in range(got.steps):
        for rank, (a, b) in enumerate(zip(got[step], ref[step])):
            ga, gb_ = a["grads"], b["grads"]
            assert ga.keys() == gb_.keys()
            pattern = sorted(n for n in ga if (ga[n] is None) != (gb_[n] is None))
            both = [n for n in ga if ga[n] is not None and gb_[n] is not None]
            found = {"gradient": _differ({n: ga[n] for n in both}, {n: gb_[n] for n in both}), "none_pattern": pattern,
                     "parameter": _differ(a["params"], b["params"]), "buffer": _differ(a["buffers"], b["buffers"])}
            out.update({(step, rank, kind): names for kind, names in found.items() if names})
    return out


def between_ranks(saved, what):
    """-> per step, the names of ``what`` ("params", "buffers", "grads") whose bits differ between rank 0 and rank 1."""
    out = []
    for step in range(saved.steps):
        a, b = saved[step]
        if what == "grads":
            a_, b_ = ({n: (torch.zeros(0) if g is None else g) for n, g in x["grads"].items()} for x in (a, b))
            out.append(_differ(a_, b_))
        else:
            out.append(_differ(a[what], b[what]))
    return out


def counts(saved):
    """-> (parameters, buffers, steps) a comparison of ``saved`` covers."""
    first = saved[0][0]
    return len(first["params"]), len(first["buffers"]), saved.steps


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank_main(config(json.loads(a.cfg)), a.out)
