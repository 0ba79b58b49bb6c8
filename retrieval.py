"""python retrieval.py with model=... checkpoint=... run_file=... ...

The reference's `retrieval.py rerank` (BM25F run of DBpedia-Entity v2 re-ranked with BLP entity embeddings, the mixing weight
alpha chosen per fold by nDCG@100) on the MI355X-native path: same config keys and defaults (retrieval.py:41-54), same log
lines, same outputs (output/{id}.run and the entity-embedding cache {run_file_name}-qent-{checkpoint name} beside the
checkpoint, interchangeable with the reference's), with
  * the entity table built through the models' encode_into (fused HIP table build on a GPU),
  * the cosines and every (alpha, query) nDCG on the device in two launches (blp_amd.ops.rerank_cosine / rerank_ndcg), the
    fold means in numpy; on a CPU the bit-exact numpy restatement (blp_amd.retrieval) -- both write the same run file,
  * trec_eval's ndcg_cut restated (blp_amd.retrieval; pytrec_eval is not needed),
  * Sacred itself if installed, otherwise blp_amd.sacred_shim.
Extra config keys: data_root (default 'data': where glove/ lives for the GloVe models), eval_dropout.
One intended divergence: the reference never calls .eval() on its encoder, so a BERT encoder's dropout is live and every query
is encoded afresh for each (alpha, fold).  Here eval_dropout=True (default) keeps the train-mode encoder but encodes each
query ONCE; eval_dropout=False puts the encoder in eval mode, which makes the whole command deterministic.
The two metrics are logged in a fixed order (ndcg_cut_10, then ndcg_cut_100; the reference iterates a set).
"""
import os
import os.path as osp

import numpy as np
import torch

try:
    from sacred import Experiment
    from sacred.observers import MongoObserver
except ImportError:  # Sacred is not in this image
    from blp_amd.sacred_shim import Experiment
    MongoObserver = None

from blp_amd import retrieval, utils
from blp_amd.data import DROPPED, GloVeTokenizer, _word_tokenize

OUT_PATH = 'output/'
device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')

ex = Experiment()
ex.logger = utils.get_logger()
if MongoObserver is not None and all([os.environ.get('DB_URI'), os.environ.get('DB_NAME')]):
    ex.observers.append(MongoObserver(os.environ['DB_URI'], os.environ['DB_NAME']))

ENCODER_NAME = 'bert-base-cased'
QUERY_MAX_LEN = 64  # retrieval.py:146-147


def remove_stopwords(text):
    return ' '.join(t for t in _word_tokenize(text) if t.lower() not in DROPPED)


@ex.config
def config():
    dim = 128
    model = 'bert-dkrl'
    rel_model = 'transe'
    max_len = 64
    emb_batch_size = 512
    checkpoint = 'output/model-348.pt'
    run_file = 'data/DBpedia-Entity/runs/v2/bm25f-ca_v2.run'
    queries_file = 'data/DBpedia-Entity/collection/v2/queries-v2_stopped.txt'
    descriptions_file = 'data/DBpedia-Entity/runs/v2/' \
                        'bm25f-ca_v2-descriptions.txt'
    qrels_file = 'data/DBpedia-Entity/collection/v2/qrels-v2.txt'
    folds_file = 'data/DBpedia-Entity/collection/v2/folds/all_queries.json'
    data_root = 'data'
    eval_dropout = True  # True: the reference's train-mode encoder (each query drawn once); False: eval mode, deterministic


def _batch_tokens(tokenizer, batch, max_len):
    if isinstance(tokenizer, GloVeTokenizer):
        enc = tokenizer.batch_encode_plus(batch, max_length=max_len)
    else:
        enc = tokenizer(batch, max_length=max_len, padding='max_length', truncation=True, return_token_type_ids=False,
                        return_tensors='pt')
    return enc['input_ids'].to(device), enc['attention_mask'].float().to(device)


def _query_tokens(tokenizer, query):
    if isinstance(tokenizer, GloVeTokenizer):
        return tokenizer.encode(query, max_length=QUERY_MAX_LEN, return_tensors='pt')
    return tokenizer.encode(query, max_length=QUERY_MAX_LEN, truncation=True, return_tensors='pt')


def load_encoder(model, dim, rel_model, checkpoint, data_root, eval_dropout, _log):
    """utils.get_model's encoder with the checkpoint's weights (saved with or without DataParallel's "module." prefix); the
    relation embeddings are dropped (retrieval.py:79-92)."""
    encoder = utils.text_model(model, dim, rel_model, 'margin', 0, 1, ENCODER_NAME, 0.0, data_root)
    state = torch.load(checkpoint, map_location='cpu')
    state = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in state.items()}
    state.pop('rel_emb.weight', None)
    result = encoder.load_state_dict(state, strict=False)
    if not set(state) - set(result.unexpected_keys):
        _log.warning(f'No parameter of {checkpoint} matches the {model} encoder: it keeps its initial weights')
    encoder = encoder.to(device)
    for param in encoder.parameters():
        param.requires_grad = False
    if not eval_dropout:
        encoder.eval()
    return encoder


@ex.capture
def embed_entities(dim, model, rel_model, max_len, emb_batch_size, checkpoint, run_file, descriptions_file, data_root,
                   eval_dropout, drop_stopwords, _log):
    tokenizer = utils.text_tokenizer(model, ENCODER_NAME, data_root)
    encoder = load_encoder(model, dim, rel_model, checkpoint, data_root, eval_dropout, _log)
    entity2idx, texts = retrieval.read_descriptions(descriptions_file)

    run_file_name = osp.splitext(osp.basename(run_file))[0]
    qent_checkpoint = osp.join(osp.dirname(checkpoint), f'{run_file_name}-qent-{osp.basename(checkpoint)}')
    if osp.exists(qent_checkpoint):
        _log.info(f'Loading entity embeddings from {qent_checkpoint}')
        return torch.load(qent_checkpoint, map_location=device), entity2idx, encoder, tokenizer

    chunks = []
    with torch.no_grad():
        for lo in range(0, len(texts), emb_batch_size):
            batch = texts[lo:lo + emb_batch_size]
            if drop_stopwords:
                batch = [remove_stopwords(t) for t in batch]
            tokens, masks = _batch_tokens(tokenizer, batch, max_len)
            out = torch.empty((len(batch), encoder.dim), dtype=torch.float32, device=device)
            encoder.encode_into(out, tokens, masks)
            chunks.append(out)
    ent_embeddings = torch.cat(chunks) if chunks else torch.empty((0, encoder.dim), device=device)
    torch.save(ent_embeddings, qent_checkpoint)
    _log.info(f'Saved entity embeddings to {qent_checkpoint}')
    return ent_embeddings, entity2idx, encoder, tokenizer


def encode_queries(query_ids, id2query, tokenizer, encoder, drop_stopwords):
    """Each query once (retrieval.py:143-152 encodes it per (alpha, fold))."""
    rows = []
    with torch.no_grad():
        for query_id in query_ids:
            query = id2query[query_id]
            if drop_stopwords:
                query = remove_stopwords(query)
            rows.append(encoder.encode(_query_tokens(tokenizer, query).to(device), text_mask=None).reshape(-1).float())
    return torch.stack(rows) if rows else torch.empty((0, encoder.dim), device=device)


@ex.automain
def rerank(model, rel_model, run_file, queries_file, qrels_file, folds_file, _run, _log):
    drop_stopwords = model in {'bert-bow', 'bert-dkrl', 'glove-bow', 'glove-dkrl'}
    ent_embeddings, entity2idx, encoder, tokenizer = embed_entities(drop_stopwords=drop_stopwords)

    id2query = retrieval.read_queries(queries_file)
    baseline_run = retrieval.read_run(run_file)
    qrels = retrieval.read_qrels(qrels_file)
    folds = retrieval.read_folds(folds_file)
    baseline_run, qrels = retrieval.restrict_to_folds(folds, baseline_run, qrels)

    problem = retrieval.pack(baseline_run, entity2idx, qrels)
    queries = encode_queries(problem.query_ids, id2query, tokenizer, encoder, drop_stopwords)
    on_device = device.type == 'cuda'
    if on_device:
        from blp_amd import ops
        s1 = ops.rerank_cosine(ent_embeddings.float().to(device), queries.to(device),
                               torch.as_tensor(problem.cand_ptr).to(device), torch.as_tensor(problem.cand_row).to(device))
    else:
        s1 = retrieval.cosine_restated(ent_embeddings.float().numpy(), queries.numpy(), problem.cand_ptr, problem.cand_row)

    # Choose best reranking on training set
    alpha_choices = np.linspace(0, 1, 20)
    search = retrieval.alpha_search(problem, s1, alpha_choices, folds, device=device if on_device else None)
    for i, fold in enumerate(search['folds']):
        best_result, best_alpha = fold['train'], fold['alpha']
        _log.info(f'[Fold {i + 1}/{len(folds)}]'
                  f' Best training result: {best_result:.3f}'
                  f' with alpha={best_alpha:.3}')
        _log.info(f'Test fold result: {fold["test"]:.3f}')

    _log.info('Finished hyperparameter search')
    _log.info('Saving run file')
    os.makedirs(OUT_PATH, exist_ok=True)
    s1_host = s1.cpu().numpy() if isinstance(s1, torch.Tensor) else s1
    test_run = retrieval.rerank_run(problem, s1_host, search['query_alpha'], alpha_choices)
    output_run_path = osp.join(OUT_PATH, f'{_run._id}.run')
    retrieval.write_run(output_run_path, test_run, model, rel_model)

    results = {}
    for metric in retrieval.METRICS:
        first_scores, second_scores = search['baseline'][metric], search['test'][metric]
        baseline_mean, test_mean = np.mean(first_scores), np.mean(second_scores)
        _log.info(f'Metric: {metric}')
        _log.info(f'Baseline result: {baseline_mean:.3f}')
        _log.info(f'Test result: {test_mean:.3f}')
        try:
            import scipy.stats
            _log.info(scipy.stats.ttest_rel(first_scores, second_scores))
        except ImportError:
            pass
        results[metric] = {'baseline': float(baseline_mean), 'test': float(test_mean)}
    results['folds'] = [{'alpha': float(f['alpha']), 'train': float(f['train']), 'test': float(f['test'])}
                        for f in search['folds']]
    results['run_file'] = output_run_path
    return results
