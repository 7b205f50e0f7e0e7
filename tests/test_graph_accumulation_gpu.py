"""GPU: gradient accumulation inside the captured training step (DenoiserTrainer(accumulation_steps=K).enable_graph on a list of K
micro-batches: vq-video-diffusion/main.py:221, :274-280 as ONE hipGraph per optimizer step).

Method and bounds are those of test_train_gpu.py::test_graphed_training_step_matches_eager, the project's "captured == eager":
loss 2e-5 relative in fp32 / 2e-2 in bf16, grad norm 1e-3 / 5e-2, weights after the trajectory rtol 1e-4 + atol 1e-6 in fp32 /
atol 3e-3 in bf16; the small model is that test's (data_shape (3,16,16), dim 256, depth 2, extents (1,1,1), C = 64)."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64
K = 2


def _bounds(dtype):
    fp32 = dtype == torch.float32
    return (2e-5 if fp32 else 2e-2), (1e-3 if fp32 else 5e-2), (dict(rtol=1e-4, atol=1e-6) if fp32 else dict(rtol=0, atol=3e-3))


def _make(seed=9, dim=256, mlp=256, depth=2):
    from world_modelz_amd import main
    torch.manual_seed(seed)
    return main.VqVideoDiffusionModel(data_shape=(3, 16, 16), dim=dim, num_classes=C, extents=(1, 1, 1), depth=depth, dim_head=128,
                                      mlp_dim=mlp, heads=1).cuda()


def _clips(n, seed=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, C, (n, 3, 16, 16), generator=g).cuda()


class Zero:
    """r = 0: the corruption is the identity, graphed and eager trainers see the same inputs."""
    def sample(self, n, generator=None): return torch.zeros(n)
    def update_with_losses(self, *a): pass


class Recording:
    """Hands out r = 0.7 and stores what it is given back."""
    def __init__(self):
        self.handed, self.given = [], []

    def sample(self, n, generator=None):
        self.handed.append(torch.full((n,), 0.7))
        return self.handed[-1]

    def update_with_losses(self, ts, losses):
        self.given.append((ts, losses.detach().clone()))


def _trainer(model, k=K, **kw):
    from world_modelz_amd import train
    kw = dict(dict(lr=1e-3, warmup=2, max_steps=100, distributed=False), **kw)
    return train.DenoiserTrainer(model, C, accumulation_steps=k, **kw)


def _same_trajectory(ta, tb, batch_a, batch_b, steps, dtype, what, r_a=None, r_b=None):
    """`steps` optimizer steps of both trainers: loss and grad norm per step, the weights at the end."""
    lb_, gb_, wtol = _bounds(dtype)
    for it in range(steps):
        la, ga = ta.train_step(batch_a, r=r_a)
        lb, gb = tb.train_step(batch_b, r=r_b)
        print(f'[{what} {dtype} step {it}] loss {la:.7f} vs {lb:.7f}, grad norm {ga:.6f} vs {gb:.6f}')
        assert abs(la - lb) < lb_ * max(1.0, abs(la)), (what, it, la, lb)
        assert abs(ga - gb) < gb_ * max(1.0, abs(ga)), (what, it, ga, gb)
    assert ta.step_count == tb.step_count == steps
    worst = max(float((a - b).abs().max()) for a, b in zip(ta.model.parameters(), tb.model.parameters()))
    print(f'[{what} {dtype}] largest weight difference after {steps} steps {worst:.3e}')
    for (n, a), b in zip(ta.model.named_parameters(), tb.model.parameters()):
        assert torch.allclose(a, b, **wtol), (what, n)


def test_enable_graph_takes_the_micro_batches_of_one_optimizer_step():
    from world_modelz_amd import config
    z = _clips(4)
    with config.compute_dtype(torch.bfloat16):
        tg = _trainer(_make())
        tg.sampler = Zero()
        assert tg.enable_graph([z[:2], z[2:]], warmup=1) is tg
        assert tg._graph is not None
        assert tuple(tg._g_z.shape) == (K, 2, 3, 16, 16)            # the clips of all micro-batches: one buffer
        assert tg._g_in.numel() == K * 2 + 3 and tg._g_in_host.numel() == K * 2 + 3 and tg._g_in_host.is_pinned()
        loss, gn = tg.train_step([z[:2], z[2:]])
        assert loss == loss and gn > 0 and tg.step_count == 1
        assert tg._g_out.numel() == 2 + K * 2                       # loss_sum, sqnorm, the K x B per-sample losses


def test_warm_up_leaves_no_trace():
    from world_modelz_amd import config
    z = _clips(4)
    with config.compute_dtype(torch.bfloat16):
        tg = _trainer(_make())
        tg.enable_ema(0.9)
        p_before, e_before = tg.arena.flat_param.clone(), tg.ema_flat.clone()
        gen_before = tg.sampler_gen.get_state().clone()
        tg.enable_graph([z[:2], z[2:]], warmup=2)                   # (the trainer's own sampler: the warm-up draws from the generator)
        assert torch.equal(tg.arena.flat_param, p_before) and tg.step_count == 0
        assert float(tg.m.abs().sum()) == 0 and float(tg.v.abs().sum()) == 0
        assert torch.equal(tg.sampler_gen.get_state(), gen_before)
        assert torch.equal(tg.ema_flat, e_before)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_graphed_accumulation_matches_the_eager_accumulation_step(dtype):
    from world_modelz_amd import config
    z = _clips(4)
    micro = [z[:2], z[2:]]
    with config.compute_dtype(dtype):
        te, tg = _trainer(_make()), _trainer(_make())
        te.sampler, tg.sampler = Zero(), Zero()
        tg.enable_graph(micro, warmup=2)
        _same_trajectory(te, tg, micro, micro, 5, dtype, 'graph K=2 vs eager K=2')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_graphed_accumulation_equals_the_graphed_union_batch(dtype):
    """main.py's 1/K scaling end to end through the graph: K = 2 x 2 clips against K = 1 on the 4 clips."""
    from world_modelz_amd import config
    z = _clips(4)
    micro = [z[:2], z[2:]]
    with config.compute_dtype(dtype):
        t1, tk = _trainer(_make(), k=1), _trainer(_make())
        t1.sampler, tk.sampler = Zero(), Zero()
        t1.enable_graph(z, warmup=2)
        tk.enable_graph(micro, warmup=2)
        _same_trajectory(t1, tk, z, micro, 5, dtype, 'graph K=1 x 4 clips vs graph K=2 x 2 clips', r_a=torch.zeros(4))


def test_every_micro_batch_of_every_replay_draws_a_fresh_corruption():
    from world_modelz_amd import config
    z = _clips(2)
    micro = [z, z.clone()]                                          # the SAME clips in both micro-batches
    with config.compute_dtype(torch.bfloat16):
        tg = _trainer(_make(), lr=0.0, warmup=0)                    # lr 0: the weights stay, only the corruption can move a loss
        tg.enable_graph(micro, warmup=1)
        rec = tg.sampler = Recording()
        ctr = [int(tg._g_ctr)]
        for _ in range(3):
            tg.train_step(micro)
            ctr.append(int(tg._g_ctr))
        assert len(rec.handed) == 3 * K and len(rec.given) == 3 * K            # K calls per step ...
        for h, (ts, losses) in zip(rec.handed, rec.given):                    # ... each with the r of its micro-batch, in order
            assert ts is h and losses.shape == (2,)
        for s in range(3):
            a, b = rec.given[K * s][1], rec.given[K * s + 1][1]
            print(f'[fresh corruption] replay {s}: per-sample losses {a.tolist()} | {b.tolist()}')
            assert not torch.equal(a, b)                                       # two streams within one replay
            if s:
                assert not torch.equal(a, rec.given[K * (s - 1)][1]) and not torch.equal(b, rec.given[K * (s - 1) + 1][1])
        assert ctr[0] >= (1 << 39)                                             # the replays' own range of Philox stream ids
        assert [c1 - c0 for c0, c1 in zip(ctr, ctr[1:])] == [K] * 3            # one stream per micro-batch, none reused
        tg.enable_graph(micro, warmup=1)                                       # capturing again does not restart the counter
        assert int(tg._g_ctr) > ctr[-1]


def test_replay_really_replays_and_everything_else_is_the_eager_step():
    from world_modelz_amd import config, sparse_diffusion, train
    z = _clips(6)
    micro = [z[:2], z[2:4]]
    with config.compute_dtype(torch.bfloat16):
        tg = _trainer(_make())
        tg.sampler = Zero()
        with pytest.raises(ValueError, match='list of 2'):
            tg.enable_graph(z[:2])                                  # a single tensor with K = 2
        with pytest.raises(ValueError, match='one shape'):
            tg.enable_graph([z[:2], z[2:5]])
        assert tg._graph is None
        tg.enable_graph(micro, warmup=1)

        class Reached(Exception):
            pass

        def eager_only(*a, **k):
            raise Reached()
        tg.forward_backward = eager_only
        loss, gn = tg.train_step(micro)                             # the graph: forward_backward is not called
        assert loss == loss and gn > 0
        loss, gn = tg.train_step(micro, r=[torch.zeros(2), torch.zeros(2)])
        assert loss == loss and tg.step_count == 2
        with pytest.raises(Reached):
            tg.train_step([z[:3], z[3:]])                           # another clip shape: the eager accumulation step
        # (three micro-batches are the eager step's too: it refuses the count before it reaches forward_backward)
        with pytest.raises(AssertionError, match='expected 2 micro-batches'):
            tg.train_step([z[:2], z[2:4], z[4:]])
        # the sparse trainer has no accumulation step, eager or captured (minecraft/sparse_diffusion.py has no such option)
        torch.manual_seed(3)
        ms = sparse_diffusion.VqSparseDiffusionModel(shape=(4, 8, 8), dim=64, num_classes=40, depth=2, dim_head=32, mlp_dim=96,
                                                     heads=2).cuda()
        tsp = train.SparseDenoiserTrainer(ms, 40, num_context=16, distributed=False, accumulation_steps=2)
        zs = torch.randint(0, 40, (2, 4, 8, 8), device='cuda')
        for example in (zs, [zs, zs]):
            with pytest.raises(NotImplementedError, match='SparseDenoiserTrainer'):
                tsp.enable_graph(example)
        assert tsp._graph is None


@contextlib.contextmanager
def _fused_backward(on):
    from world_modelz_amd import config
    prev = config.fused_backward()
    config.set_fused_backward(on)
    try:
        yield
    finally:
        config.set_fused_backward(prev)


def test_chain_widths_accumulate_in_the_graph():
    """bf16 on a width of csrc/chain_widths.h (dim 96 / 1 x 128 / mlp 256), chain kernels forced: the ChainPackSet is refreshed
    once per replay.  (The weight bound is the default widths': the existing data-parallel capture test holds dim 96 to it.)"""
    from conftest import chain_policy, recorded_calls
    from world_modelz_amd import config, fused
    z = _clips(4)
    micro = [z[:2], z[2:]]
    with config.compute_dtype(torch.bfloat16), chain_policy('always'):
        te, tg = _trainer(_make(dim=96)), _trainer(_make(dim=96))
        assert tg.chain_packs is not None
        assert fused.training_route(tg.model.transformer, torch.bfloat16, micro[0].numel(), True) == ('chain', True)
        te.sampler, tg.sampler = Zero(), Zero()
        with recorded_calls() as seen:
            tg.enable_graph(micro, warmup=0)
        assert any('chain' in name and 'bwd' in name for name in seen), sorted(set(seen))
        _same_trajectory(te, tg, micro, micro, 3, torch.bfloat16, 'chain width, graph K=2 vs eager K=2')


def test_fused_forward_under_the_op_by_op_backward_accumulates_in_the_graph():
    from world_modelz_amd import config
    z = _clips(4)
    micro = [z[:2], z[2:]]
    with config.compute_dtype(torch.bfloat16), _fused_backward(False):
        te, tg = _trainer(_make()), _trainer(_make())
        assert tg.packs is None
        te.sampler, tg.sampler = Zero(), Zero()
        tg.enable_graph(micro, warmup=1)
        _same_trajectory(te, tg, micro, micro, 3, torch.bfloat16, 'fused_backward off, graph K=2 vs eager K=2')


def test_weight_ema_moves_once_per_optimizer_step():
    from world_modelz_amd import config
    z = _clips(4)
    micro = [z[:2], z[2:]]
    with config.compute_dtype(torch.bfloat16):
        te, tg = _trainer(_make()), _trainer(_make())
        te.sampler, tg.sampler = Zero(), Zero()
        te.enable_ema(0.5)
        tg.enable_ema(0.5)
        # the shadow weights start 1.0 away from the weights: after three updates at decay 0.5 an eighth of that is left, after six
        # (one per micro-batch) a sixty-fourth -- 0.11 apart, where the weights themselves move by ~1e-3 a step
        te.ema_flat.add_(1.0)
        tg.ema_flat.add_(1.0)
        e0 = tg.ema_flat.clone()
        tg.enable_graph(micro, warmup=2)
        assert torch.equal(tg.ema_flat, e0)
        for _ in range(3):
            te.train_step(micro)
            tg.train_step(micro)
        d = float((te.ema_flat - tg.ema_flat).abs().max())
        left = float((tg.ema_flat - tg.arena.flat_param).mean())
        print(f'[ema] graphed vs eager {d:.3e}; mean distance from the weights {left:.4f} (1/8 = 0.125)')
        assert torch.allclose(te.ema_flat, tg.ema_flat, rtol=0, atol=3e-3)
        assert abs(left - 0.125) < 1e-2


# ---- data parallel: RCCL world of one, in a fresh child process ---------------------------------------------------------------------
def test_data_parallel_accumulation_is_captured_on_rccl_world_of_one():
    """The reducer is built with rounds = K: under capture every bucket's all-reduce is a node behind the LAST micro-batch's
    backward, finish() the one join.  In a FRESH child process (an abort inside an RCCL-capturing capture would take the tests
    behind it down), under its own time limit; a child that died or hung ends the session -- nothing more starts on that GPU."""
    if os.environ.get('WMZ_RCCL_CHILD') == '1':
        return _data_parallel_body()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, '-m', 'pytest', f'{os.path.abspath(__file__)}::test_data_parallel_accumulation_is_captured_on_rccl_world_of_one',
           '-m', 'gpu', '-q', '-s', '-p', 'no:cacheprovider']
    try:
        r = subprocess.run(cmd, env=dict(os.environ, WMZ_RCCL_CHILD='1', HSA_ENABLE_IPC_MODE_LEGACY='0'), capture_output=True,
                           text=True, timeout=600, cwd=root)
    except subprocess.TimeoutExpired:
        pytest.exit('the data-parallel capture child ran into its time limit: nothing more is started on this GPU', returncode=3)
    for line in r.stdout.splitlines():
        if line.startswith('['):
            print(line)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f'the data-parallel capture child died (exit {r.returncode}): nothing more is started on this GPU\n'
                    + r.stderr[:3000] + '\n...\n' + r.stderr[-1500:], returncode=3)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[:3000] + '\n...\n' + r.stderr[-1500:]


def _data_parallel_body():
    import gc
    import torch.distributed as dist
    from world_modelz_amd import config
    if dist.is_initialized():
        pytest.skip('a process group already exists in this process')
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29547')
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    trainers = []
    try:
        z = _clips(4)
        micro = [z[:2], z[2:]]
        for dtype in (torch.bfloat16, torch.float32):               # the fused kernels' in-place gradients; autograd's, op by op
            with config.compute_dtype(dtype):
                te, tg = _trainer(_make(depth=3), distributed=True), _trainer(_make(depth=3), distributed=True)
                ts = _trainer(_make(depth=3))
                trainers += [te, tg, ts]
                for t in (te, tg, ts):
                    t.sampler = Zero()
                red = tg.reducer
                assert red is not None and red.active and red.world == 1 and red.rounds == K and len(red.buckets) == 3 + 2
                # what happens in which order while the step body runs: micro-batch boundaries, collectives, the join
                events = []
                step, launch, finish = tg._graph_step, red._launch, red.finish

                def graph_step(*a, **k):
                    out = step(*a, **k)
                    events.append('micro-batch done')
                    return out

                def _launch(b):
                    events.append(('all-reduce', b, torch.cuda.is_current_stream_capturing()))
                    return launch(b)

                def _finish():
                    out = finish()                                  # (buckets the backward left behind are launched in here)
                    events.append('finish')
                    return out
                tg._graph_step, red._launch, red.finish = graph_step, _launch, _finish
                try:
                    tg.enable_graph(micro, warmup=1)
                finally:
                    tg._graph_step, red._launch, red.finish = step, launch, finish
                assert tg._graph is not None and tg.step_count == 0
                bodies = [i for i, e in enumerate(events) if e == 'finish']
                assert len(bodies) == 2                                                        # one warm-up body, the captured one
                body = events[bodies[0] + 1:bodies[1] + 1]
                assert body.count('micro-batch done') == K and body[-1] == 'finish'
                first_done = body.index('micro-batch done')
                reduces = [e for e in body if isinstance(e, tuple)]
                assert not any(isinstance(e, tuple) for e in body[:first_done + 1]), body    # none behind the first micro-batch
                assert sorted(b for _, b, _ in reduces) == list(range(5)) and all(cap for _, _, cap in reduces), body
                if dtype == torch.bfloat16:
                    # the fused backward announces its gradients itself: every bucket leaves inside the LAST backward, head first
                    last_done = len(body) - 1 - body[::-1].index('micro-batch done')
                    assert all(isinstance(e, tuple) for e in body[first_done + 1:last_done]) and last_done == len(body) - 2, body
                    assert reduces[0][1] == 4 and reduces[-1][1] == 0
                assert sorted(red.last_order) == list(range(5))
                lb_, gb_, wtol = _bounds(dtype)
                ts.enable_graph(micro, warmup=1)                    # the single-process graphed K-step
                for it in range(3):
                    le, ge = te.train_step(micro)
                    lg, gg = tg.train_step(micro)
                    ls, gs = ts.train_step(micro)
                    print(f'[ddp accumulation {dtype} step {it}] eager {le:.7f} / {ge:.6f}, graph {lg:.7f} / {gg:.6f}, '
                          f'single-process graph {ls:.7f} / {gs:.6f}')
                    assert abs(le - lg) < lb_ * max(1.0, abs(le)) and abs(ls - lg) < lb_ * max(1.0, abs(ls)), (it, le, lg, ls)
                    assert abs(ge - gg) < gb_ * max(1.0, abs(ge)) and abs(gs - gg) < gb_ * max(1.0, abs(gs)), (it, ge, gg, gs)
                assert te.step_count == tg.step_count == ts.step_count == 3
                for (n, a), b, c in zip(te.model.named_parameters(), tg.model.parameters(), ts.model.parameters()):
                    assert torch.allclose(a, b, **wtol) and torch.allclose(c, b, **wtol), (dtype, n)
                for t in (te, tg, ts):
                    t._graph = None
                torch.cuda.synchronize()
    finally:
        # (captured graphs hold RCCL kernels: let go of them and drain the device before the communicator is torn down)
        for t in trainers:
            t._graph = None
        gc.collect()
        torch.cuda.synchronize()
        dist.destroy_process_group()
