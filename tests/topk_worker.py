"""Worker of tests/test_topk_host.py::test_sharded_predict_links_equals_unsharded, one process per gloo rank: the entity
table sharded along the candidate axis (ranking.shard_bounds), every rank answers the same filtered queries from its own
rows, and ranking.predict_links merges the ranks' lists (one all-gather).  Each rank saves what it got."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, T, K, R = 203, 128, 9, 12, 5


def problem(rel_model):
    from blp_amd import models, utils
    gen = torch.Generator().manual_seed(7)
    model = models.LinkPrediction(D, rel_model, "margin", R, 0)
    with torch.no_grad():
        model.rel_emb.weight.copy_((torch.rand(R, D, generator=gen) - 0.5) * 0.25)
    table = torch.randn(N, D, generator=gen)
    table = torch.nn.functional.normalize(table, dim=-1) if rel_model == "transe" else table * 0.1
    table[40:60] = table[20]  # duplicates: equal scores across shard boundaries
    entities = torch.randperm(N, generator=gen) + 1000
    ent2idx = utils.make_ent2idx(entities, int(entities.max()))
    triples = torch.stack((entities[torch.randint(0, N, (T,), generator=gen)], entities[torch.randint(0, N, (T,), generator=gen)],
                           torch.randint(0, R, (T,), generator=gen)), dim=1)
    edges = torch.stack((entities[torch.randint(0, N, (600,), generator=gen)], entities[torch.randint(0, N, (600,), generator=gen)],
                         torch.randint(0, R, (600,), generator=gen)), dim=1)
    edges = torch.cat((edges, triples))
    return model, table, triples, ent2idx, utils.FilterIndex(edges), entities


def unsharded(rel_model):
    from blp_amd import ranking
    model, table, triples, ent2idx, index, entities = problem(rel_model)
    return ranking.predict_links(model, table, triples, K, ent2idx, filter_index=index, entities=entities)


def run(rank, world, port, rel_model, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from blp_amd import ranking
        model, table, triples, ent2idx, index, entities = problem(rel_model)
        lo, hi = ranking.shard_bounds(N, world, rank)
        rows, scores = ranking.predict_links(model, table[lo:hi].clone(), triples, K, ent2idx, filter_index=index,
                                             entities=entities, world=world, rank=rank, num_entities=N)
        np.save(os.path.join(out_dir, f"rows_{rank}.npy"), rows.numpy())
        np.save(os.path.join(out_dir, f"scores_{rank}.npy"), scores.numpy())
    finally:
        dist.destroy_process_group()
