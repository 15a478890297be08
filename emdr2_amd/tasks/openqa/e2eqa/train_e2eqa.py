"""Training-step driver of the QA task (reference: tasks/openqa/e2eqa/train_e2eqa.py:28-41,126-181 and
megatron/training.py:165-230).  Same forward-step contract: forward_step(batch_or_iter, model) -> (loss, {'lm_loss', 'retriever_loss'})."""
import json
import os
import time

import torch

from emdr2_amd import checkpointing
from emdr2_amd.global_vars import get_args
from emdr2_amd.model.emdr2_model import emdr2_loss
from emdr2_amd.tasks.openqa.e2eqa.eval_utils import exact_match_score, metric_max_over_ground_truths
from emdr2_amd.tasks.openqa.e2eqa.train_data_utils import collate
from emdr2_amd.training import AnnealingLR, allreduce_gradients


def process_batch(batch):
    dev = "cuda"
    return (batch['query_uid'].to(dev), batch['query_ids_bert'].to(dev), batch['query_types'].to(dev), None,
            batch['query_ids_t5'].to(dev), batch['query_ids_t5_len'].to(dev), batch['dec_ids'].to(dev), batch['labels'].to(dev),
            batch['loss_mask'].to(dev), batch.get('reference'))


def _cross_entropy_forward_step(batch, model, eos_id):
    try:
        batch_ = next(batch)
    except BaseException:
        batch_ = batch
    query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len, dec_ids, labels, loss_mask, reference = process_batch(batch_)
    assert torch.all(query_uid < 0), "query uid can't be positive"
    tracker = getattr(model, "answer_hits", None)
    if tracker is not None and model.training:                # --retrieval-answer-hits: what this step's retrieval is matched against
        tracker.begin(batch_['query_uid'].tolist(), reference)
    meter = getattr(model, "reader_mass", None)
    if meter is not None and model.training:                  # --reader-attention-mass: the groups of this step add to it
        meter.begin()
    try:
        ret_kldiv, micro = bool(getattr(get_args(), 'ret_kldiv', False)), int(getattr(get_args(), 'question_micro_batches', 1) or 1)
    except RuntimeError:
        ret_kldiv, micro = False, 1
    if micro > 1 and model.training:
        # --question-micro-batches: forward, loss and backward per group of questions inside the model; the returned loss carries no graph
        # (train_step skips its backward call)
        net_loss, stats = model.forward_backward(query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len, dec_ids, labels, loss_mask, eos_id,
                                                 micro_batches=micro, ret_kldiv=ret_kldiv)
        return net_loss, {'lm_loss': stats['lm_loss'], 'retriever_loss': stats['retriever_loss']}
    lm_logits, topk_log_probs, lm_logits_one_context = model(query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len, dec_ids)
    net_loss, stats = emdr2_loss(lm_logits, topk_log_probs, lm_logits_one_context, labels, loss_mask, eos_id, ret_kldiv=ret_kldiv)
    return net_loss, {'lm_loss': stats['lm_loss'], 'retriever_loss': stats['retriever_loss']}


def train_step(forward_step_func, data_iterator, model, optimizer, lr_scheduler, eos_id, dp_group=None, guard=None):
    """megatron/training.py:202-230 without the loss scale (bf16 needs none).  The other half of the fp16 machinery, never applying a step
    whose gradients are non-finite (fp16/fp16.py:420-474), is the optimizer's: FlatAdam(skip_nonfinite=True), --skip-nonfinite-steps,
    decides it on the device, and the schedule below advances either way.  `guard` (training.RetentionGuard,
    built when --recompute-keep-last-layers / --selective-retention-layers ask for activations to be kept or --question-micro-batches
    splits the step): a step that runs out of HBM is run again on all ranks together, with a thinner retention plan / a finer split if
    need be, instead of ending the job."""
    from emdr2_amd.model import kernels
    try:
        batch = next(data_iterator)                  # fetched once: a re-run of the step sees the same batch
    except TypeError:
        batch = data_iterator

    def step_once():
        optimizer.zero_grad()
        sink = kernels.GRAD_SINK
        if sink is not None and sink is not optimizer:
            sink.begin_step()
        loss, loss_reduced = forward_step_func(batch, model, eos_id)
        if loss.requires_grad:                       # (a micro-batched forward step has already back-propagated, group by group)
            loss.backward()
        if sink is not None:
            sink.finish()                            # buckets were all-reduced (bf16, pre-divided) while the backward ran
        else:
            allreduce_gradients(model, dp_group)
        return loss_reduced
    loss_reduced = guard.run(step_once) if guard is not None else step_once()
    # the reference steps the optimizer with the rate its scheduler set at the END of the previous iteration (training.py:223-228,
    # learning_rates.py:73-80): step n runs at lr(n - 1), so the very first update of a warm-up schedule has lr 0
    optimizer.step(lr=lr_scheduler.get_lr())
    lr_scheduler.step()
    return loss_reduced


# =====================================================================================================================================
# the task driver: data loaders, evaluation callbacks, epoch loop (reference: tasks/openqa/e2eqa/train_e2eqa.py:216-621)
# =====================================================================================================================================
def print_rank_0(msg):
    if not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0:
        print(msg, flush=True)


def _dp():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank(), torch.distributed.get_world_size()
    return 0, 1


def build_data_loader(dataset, batch_size, num_workers, drop_last, shuffle=True):
    """train_e2eqa.py:343-367: per-rank batches through a DistributedSampler; the collate keeps the 10-key batch of a1."""
    rank, world = _dp()
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=shuffle)
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, sampler=sampler, shuffle=False, num_workers=num_workers,
                                       drop_last=drop_last, pin_memory=True, collate_fn=collate)


def reader_em_score(model, dataloader, topk_retrievals, tokenizer):
    """train_e2eqa.py:216-283: greedy (--beam-size 1) or beam-search answers, exact match against every reference answer, de-duplicated
    over ranks by query uid."""
    from emdr2_amd.model.search_strategy import BeamSearch, SampleOrGreedySearch
    args = get_args()
    if args.beam_size < 1:
        raise AssertionError("--beam-size < 1 is not supported for ORQA reader.")
    score_list, quid_list, best_list, read_list = [], [], [], []
    tracker = getattr(model, "answer_hits", None)            # --retrieval-answer-hits
    read = tracker is not None and getattr(model, "reader_attention_mass", False) and args.beam_size == 1    # --reader-attention-mass
    model.eval()
    with torch.no_grad():
        for batch in dataloader:
            query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len, _, _, _, reference = process_batch(batch)
            if args.beam_size == 1:
                search = SampleOrGreedySearch(max_decode_len=args.max_decode_len, bos_id=tokenizer.bos_token_id, eos_id=tokenizer.eos_token_id,
                                              sample=False, topk_evidence=topk_retrievals)
            else:
                search = BeamSearch(max_decode_len=args.max_decode_len, bos_id=tokenizer.bos_token_id, eos_id=tokenizer.eos_token_id,
                                    beam_size=args.beam_size, topk_evidence=topk_retrievals)
            hypothesis = search.generate_output(model, query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len)
            if tracker is not None:                           # the passages this batch's answers were read from
                hit_pos, best = tracker.best_slots(batch['query_uid'].tolist(), reference, model.evidence_retriever.last_kept_ids)
                best_list.append(best)
                if read:                                      # does the slot the decoder read most, over its decoding steps, hold an answer
                    top = model.last_attention_mass.argmax(dim=1)
                    read_list.append(hit_pos.gather(1, top[:, None])[:, 0] >= 0)
            for quid, ref, hyp in zip(query_uid.tolist(), reference, hypothesis):
                score_list.append(float(metric_max_over_ground_truths(exact_match_score, tokenizer.decode(hyp), ref)))
                quid_list.append(quid)
    model.train()
    scores = torch.tensor(score_list, dtype=torch.float32, device="cuda")
    quids = torch.tensor(quid_list, dtype=torch.int64, device="cuda")
    if tracker is not None:                                   # best slots travel with the scores: same padding, gather and de-duplication
        bests = torch.cat(best_list).to(torch.float32) if best_list else torch.zeros(0, device="cuda")
        cols = [scores, bests]
        if read:
            cols.append(torch.cat(read_list).to(torch.float32) if read_list else torch.zeros(0, device="cuda"))
        scores = torch.stack(cols, dim=1)
    rank, world = _dp()
    if world > 1:                                                        # ranks may hold different counts (drop_last False): pad to the max
        n = torch.tensor([scores.shape[0]], device="cuda"); nmax = n.clone()
        torch.distributed.all_reduce(nmax, op=torch.distributed.ReduceOp.MAX)
        pad = int(nmax.item()) - scores.shape[0]
        scores = torch.cat([scores, torch.zeros((pad,) + tuple(scores.shape[1:]), device="cuda")])
        quids = torch.cat([quids, torch.zeros(pad, dtype=torch.int64, device="cuda")])
        gs = [torch.empty_like(scores) for _ in range(world)]; gq = [torch.empty_like(quids) for _ in range(world)]
        torch.distributed.all_gather(gs, scores); torch.distributed.all_gather(gq, quids)
        scores, quids = torch.cat(gs), torch.cat(gq)
    score_dict = {q: s for q, s in zip(quids.tolist(), scores.tolist()) if q != 0}     # duplicates (sampler padding) overwrite
    if tracker is None:
        return {'Exact Match Score': sum(score_dict.values())}, len(score_dict)
    stats = {'Exact Match Score': sum(s[0] for s in score_dict.values())}
    for k in tracker.ks:                                      # counts, like the EM score: metrics_func prints them as percentages of the total
        stats['Answer Hits@{}'.format(k)] = sum(1 for s in score_dict.values() if s[1] < k)
    if read:
        stats['Read Top-1 Hit'] = sum(1 for s in score_dict.values() if s[2] > 0)
    return stats, len(score_dict)


def validation_loss(model, dataloader, eos_id):
    """train_e2eqa.py:286-321."""
    total, score = 0, 0.0
    model.eval()
    with torch.no_grad():
        for batch in dataloader:
            query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len, dec_ids, labels, loss_mask, _ = process_batch(batch)
            lm_logits, topk_log_probs, _, _ = model(query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len, dec_ids)
            _, stats = emdr2_loss(lm_logits, topk_log_probs, None, labels, loss_mask, eos_id)
            total += 1
            score += float(stats['lm_loss'])
    model.train()
    t = torch.tensor([score, total], dtype=torch.float32, device="cuda")
    if _dp()[1] > 1:
        torch.distributed.all_reduce(t)
    return {'Validation Loss': t[0]}, t[1]


def accuracy_func_provider(single_dataset_provider, datapath, tokenizer):
    """train_e2eqa.py:324-341."""
    args = get_args()
    if not datapath:
        return lambda model, epoch: None
    dataset = single_dataset_provider(datapath)
    dataloader = build_data_loader(dataset, args.eval_batch_size, num_workers=args.num_workers, drop_last=False, shuffle=False)

    def metrics_func(model, epoch):
        print_rank_0('calculating metrics ...')
        stats, total = reader_em_score(model, dataloader, args.topk_retrievals, tokenizer)
        fmt = "|total_questions: {}".format(total)
        for k, v in stats.items():
            fmt += "|{} = {:.2f}".format(k, (v * 100) / max(total, 1))
        print_rank_0("epoch:{}{}".format(epoch, fmt))
        return stats, total
    return metrics_func


def setup_model_and_optimizer(model_provider):
    from emdr2_amd.model import kernels as _K
    _K.PACKING.sticky = True                                  # training: packed stacks keep constant sizes from step to step (kernels._Packing)
    return _setup_model_and_optimizer(model_provider)


def _setup_model_and_optimizer(model_provider):
    """megatron/training.py:136-162: model, FusedAdam over the (decay / no-decay) groups, AnnealingLR, resume or pre-trained init."""
    args = get_args()
    model = model_provider()
    from emdr2_amd.model import kernels
    from emdr2_amd.training import FlatAdam
    # flat buckets (masters, gradients, moments, bf16 working copies), no-decay grouping of model/utils.py:64-83 inside each bucket; it is
    # also the gradient sink of the backward: data-parallel buckets are exchanged in bf16 as soon as they are complete
    optimizer = kernels.GRAD_SINK = FlatAdam(model, lr=args.lr, weight_decay=args.weight_decay, clip_grad=args.clip_grad,
                                             skip_nonfinite=bool(getattr(args, 'skip_nonfinite_steps', False)),
                                             audit_state=int(getattr(args, 'audit_optimizer_state_interval', 0) or 0) > 0)
    num_iters = args.lr_decay_iters if args.lr_decay_iters is not None else args.train_iters
    num_iters = max(1, num_iters)
    lr_scheduler = AnnealingLR(args.lr, warmup_iter=args.warmup * num_iters, total_iters=num_iters, min_lr=args.min_lr)
    no_optim = args.no_load_optim or getattr(args, 'finetune', False)                  # checkpointing.py:243-256: schedule only with the optimizer
    args.iteration = checkpointing.load_checkpoint(args.load, model, None if no_optim else optimizer, None if no_optim else lr_scheduler) if args.load else 0
    if args.iteration == 0:
        model.init_state_dict_from_dpr_and_t5(args.pretrained_t5_load, args.pretrained_dpr_load)      # training.py:156-158
    return model, optimizer, lr_scheduler


def _save(iteration, model, optimizer, lr_scheduler):
    args = get_args()
    rank, world = _dp()
    checkpointing.save_checkpoint(args.save, iteration, model, None if args.no_save_optim else optimizer, lr_scheduler, rank=rank,
                                  barrier=torch.distributed.barrier if world > 1 else None, args=args)


def index_writeback(model, batch_size, topk, generation=None, newest_wins=False, skipped=None):
    """--index-writeback, at a step boundary: the embeddings the step has just computed for the passages it retrieved
    (`EMDR2Model.take_writeback`) go into the index rows they were retrieved from (`update_rows_at`).  The list always has
    batch_size * topk entries, padded with row -1 (skipped): the short last batch of an epoch under --keep-last, empty retrieval slots,
    a step that kept nothing.  With more than one rank every rank gathers all ranks' lists -- ONE all-gather of the row numbers and ONE
    of the fp16 rows over the retriever's group, issued by every rank at every boundary so that the collective sequence stays static
    -- and applies the gathered list to its own shard: rows of other shards fall out of range there.  A passage retrieved by several
    questions holds the embedding of the last (rank, question, slot) that names it, the same on every rank.  `generation` (an index with
    generation stamps: --index-generations): the stamp of the rows, the step count of the weights the forward ran with; `newest_wins`
    (--index-newest-wins): rows that hold a newer stamp are left alone.  `skipped` (--skip-nonfinite-steps: FlatAdam.last_step_skipped, a
    device bool): every entry of a skipped step, and any entry whose embedding holds a non-finite value, becomes row -1 before the
    gather -- device arithmetic on a list of unchanged length, so the collectives are the same and no non-finite row enters the index
    through this writer."""
    retriever = model.evidence_retriever
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(batch_size) * int(topk)
    rows = torch.full((n,), -1, dtype=torch.int64, device=dev)
    embeds = torch.zeros((n, model.hidden_size), dtype=torch.float16, device=dev)
    kept = model.take_writeback()
    if kept is not None:
        rows[:kept[0].shape[0]] = kept[0]
        embeds[:kept[1].shape[0]] = kept[1]
    if skipped is not None:
        rows = torch.where(~torch.isfinite(embeds).all(1) | skipped, torch.full_like(rows, -1), rows)
    rank, world = retriever._world()
    if world > 1:
        all_rows = torch.empty((world * n,), dtype=rows.dtype, device=dev)
        all_embeds = torch.empty((world * n, embeds.shape[1]), dtype=embeds.dtype, device=dev)
        torch.distributed.all_gather_into_tensor(all_rows, rows, group=retriever.process_group)
        # (as bytes: a gather moves bits, and not every transport knows fp16)
        torch.distributed.all_gather_into_tensor(all_embeds.view(torch.uint8), embeds.view(torch.uint8), group=retriever.process_group)
        rows, embeds = all_rows, all_embeds
    if generation is None:
        retriever.mips_index.update_rows_at(rows, embeds)
    else:
        retriever.mips_index.update_rows_at(rows, embeds, generation=generation, newest_wins=newest_wins)


def skipped_step_line(report, iteration):
    """--skip-nonfinite-steps, at a --log-interval boundary: the first step skipped since the last such line (FlatAdam.guard_report)."""
    if report["parameter"] is None and not (report["nan"] or report["inf"]):
        where = "the squared gradient norm overflowed fp32 over finite elements"
    elif report["parameter"] is None:
        where = "first non-finite gradient element in no parameter's slice"
    else:
        where = "first non-finite gradient element: %s[%d]" % (report["parameter"], report["element"])
    return "skipped step at iteration %d: %s | NaN elements: %d | Inf elements: %d" % (iteration, where, report["nan"], report["inf"])


def interval_average(total, log_interval, skipped):
    """training.py:298-306: the average of an interval's losses over the steps that were applied."""
    return total / max(1, log_interval - skipped)


def writeback_generation(iteration):
    """The stamp of the rows written back at the boundary after step `iteration`: that step's forward, which computed them, ran with the
    weights of `iteration - 1` optimizer steps."""
    return max(int(iteration) - 1, 0)


def index_generation_line(index, iteration, retrieved):
    """--index-generations, at a --log-interval boundary after every writer of the boundary: one line on rank 0.  `retrieved`: the
    statistics of the rows the step's search returned, taken BEFORE the boundary's writers touched them, against the step count of the
    weights the forward ran with.  The whole index is counted now, against `iteration`.  `generation_stats` is collective over the index's
    group (two small all-reduces, at iterations that depend on --log-interval alone); `kept_newer` is one host read on this rank, and
    the count printed is rank 0's shard's.  -> the whole-index statistics."""
    whole = index.generation_stats(iteration)
    kept = index.kept_newer()
    line = "index generations at iteration %d: retrieved rows mean age %.2f max %d (%d rows) | whole index mean age %.2f max %d (%d rows) | " \
           "kept newer %d" % (iteration, retrieved["mean_age"], retrieved["max_age"], retrieved["count"], whole["mean_age"], whole["max_age"],
                              whole["count"], kept)
    if whole["from_future"]:
        line += " | %d rows stamped beyond iteration %d" % (whole["from_future"], iteration)
    print_rank_0(line)
    return whole


def save_index_delta(index, path, iteration, take_base):
    """--save-index-deltas, after a checkpoint save that is not an index update: the rows that differ from the published snapshot go to
    `path + '.delta'` (`DistributedBruteForceIndex.save_delta`; collective, one line on rank 0).  `take_base`: no refresher ever begins a
    snapshot (--index-writeback alone), so the first call takes one, synchronously, and later calls write deltas against it."""
    base = index.delta_base
    if take_base and (base is None or base.get("path") != os.path.abspath(path)):
        index.save_flat_file(path, {"iteration": iteration, "refreshes": 0, "mode": "writeback"}, track_deltas=True)
        print_rank_0("index delta: base snapshot taken at iteration {}".format(iteration))
        return None
    return index.save_delta(path, {"iteration": iteration}, log=print_rank_0)


def audit_index(index, iteration):
    """--audit-index-interval: one audit of the evidence index (`DistributedBruteForceIndex.audit`: every rank its own shard, the counters
    reduced over the index's group, so every rank holds the same result and takes the same decision).  Rank 0 prints one line; an index
    that is not sound and canonical raises RuntimeError on every rank, naming the non-zero report words and the first offender."""
    from emdr2_amd.data.emdr2_index import audit_failures
    torch.cuda.synchronize()
    t0 = time.time()
    result = index.audit()                                      # (ends with its one host read: the time below is the audit's)
    ms = (time.time() - t0) * 1000.0
    bad = audit_failures(result)
    if bad:
        print_rank_0("index audit at iteration %d: %d rows, FAILED: %s (%.2f ms)" % (iteration, result["rows_checked"], bad, ms))
        raise RuntimeError("index audit failed at iteration %d: %s" % (iteration, bad))
    print_rank_0("index audit at iteration %d: %d rows, sound, canonical (%.2f ms)" % (iteration, result["rows_checked"], ms))
    return result


def maybe_audit_index(index, iteration, interval):
    """The step-boundary rule of --audit-index-interval: audit at every iteration divisible by `interval`; 0 = never.  Whether a boundary
    audits -- and so issues the audit's collectives -- depends on the iteration number alone.  -> whether it did."""
    if interval <= 0 or iteration % interval:
        return False
    audit_index(index, iteration)
    return True


def optimizer_audit_failures(result):
    """The non-zero counts of a FlatAdam.audit() result on the worst replica, each with its first offender: '' for a sound state.  Built
    from all-reduced words, so every rank holds the same text."""
    bad = []
    for name, count in result["worst"].items():
        if count:
            parameter, element = result["worst_first"][name]
            where = "%s[%d]" % (parameter, element) if parameter is not None else "bucket element %d (padding)" % element
            bad.append("%s = %d (first: %s)" % (name, count, where))
    return ", ".join(bad)


def audit_optimizer_state(optimizer, iteration):
    """--audit-optimizer-state-interval: one audit of the optimizer state (`FlatAdam.audit`: a streaming launch per bucket, two small
    all-reduces over the data-parallel group, one host read; every rank holds the same result and takes the same decision).  Rank 0
    prints one line; a replica that differs raises RuntimeError on every rank inside the audit, an unsound state here, naming the
    non-zero counts and the first offender."""
    torch.cuda.synchronize()
    t0 = time.time()
    result = optimizer.audit()                                  # (ends with its one host read: the time below is the audit's)
    ms = (time.time() - t0) * 1000.0
    bad = optimizer_audit_failures(result)
    if bad:
        print_rank_0("optimizer state audit at iteration %d: %d elements in %d buckets, FAILED: %s (%.2f ms)"
                     % (iteration, result["elements"], result["buckets"], bad, ms))
        raise RuntimeError("optimizer state audit failed at iteration %d: %s" % (iteration, bad))
    print_rank_0("optimizer state audit at iteration %d: %d elements in %d buckets, sound, replicas identical (world %d) (%.2f ms)"
                 % (iteration, result["elements"], result["buckets"], result["world"], ms))
    return result


def maybe_audit_optimizer_state(optimizer, iteration, interval):
    """The step-boundary rule of --audit-optimizer-state-interval: audit at every iteration divisible by `interval`; 0 = never.  Whether
    a boundary audits -- and so issues the audit's collectives -- depends on the iteration number alone.  -> whether it did."""
    if interval <= 0 or iteration % interval:
        return False
    audit_optimizer_state(optimizer, iteration)
    return True


def param_stats_lines(stats, iteration, lr, clip):
    """The log lines of one FlatAdam.param_stats() result: the summary -- grad norm, params norm and num zeros over all parameters (what
    Megatron-LM logs under these names), the clip factor the step derived from that norm (min(1, clip / (norm + 1e-6)), the Adam kernel's
    expression; 1 with clipping off), the five parameters with the largest lr * |d| / |w| (the Adam part of the last update against the
    weights it moved) and the five with the largest share of the squared gradient norm -- then one line per group.  Pure."""
    from emdr2_amd.training import group_param_stats
    params = stats["params"]
    gsq, wsq = sum(r["grad_sq"] for r in params.values()), sum(r["weight_sq"] for r in params.values())
    gnorm = gsq ** 0.5
    factor = min(1.0, clip / (gnorm + 1.0e-6)) if clip and clip > 0 else 1.0
    ratio = {n: lr * r["direction_sq"] ** 0.5 / r["weight_norm"] for n, r in params.items() if r["weight_norm"] > 0}
    moved = sorted(ratio, key=lambda n: -ratio[n])[:5]
    share = sorted(params, key=lambda n: -params[n]["grad_sq"])[:5] if gsq > 0 else []
    lines = [" param stats at iteration %d (step %d, gradients %s): grad norm: %.6E | params norm: %.6E | num zeros: %d | non-finite: %d | "
             "clip factor: %.6f | largest lr*|d|/|w|: %s | largest share of grad norm^2: %s"
             % (iteration, stats["step"], "current" if stats["grads_current"] else "not current", gnorm, wsq ** 0.5,
                sum(r["grad_zeros"] for r in params.values()), sum(r["grad_nonfinite"] for r in params.values()), factor,
                ", ".join("%s %.3E" % (n, ratio[n]) for n in moved) or "-",
                ", ".join("%s %.1f%%" % (n, 100.0 * params[n]["grad_sq"] / gsq) for n in share) or "-")]
    for name, g in group_param_stats(stats).items():
        lines.append(" param stats group %s: %d tensors, %d elements | grad norm: %.6E | params norm: %.6E | direction rms: %.6E | "
                     "max abs grad: %.3E | num zeros: %d | non-finite: %d"
                     % (name, g["params"], g["n"], g["grad_norm"], g["weight_norm"], g["direction_rms"], g["max_abs_grad"], g["grad_zeros"],
                        g["grad_nonfinite"]))
    return lines


def log_param_stats(optimizer, iteration, path=None):
    """--log-param-stats-interval: one FlatAdam.param_stats() call (two launches per bucket, one host read, no collective: every rank
    would read the same bits), the lines of param_stats_lines on rank 0 and, with --param-stats-file, one appended JSON line holding
    every parameter's record."""
    stats = optimizer.param_stats()
    lr = float(getattr(optimizer, "last_lr", optimizer.lr))
    for line in param_stats_lines(stats, iteration, lr, optimizer.clip_grad):
        print_rank_0(line)
    if path and (not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0):
        with open(path, "a") as f:
            f.write(json.dumps(dict(stats, iteration=iteration, lr=lr)) + "\n")
    return stats


def maybe_log_param_stats(optimizer, iteration, interval, path=None):
    """The step-boundary rule of --log-param-stats-interval: at every iteration divisible by `interval`; 0 = never.  -> whether it did."""
    if interval <= 0 or iteration % interval:
        return False
    log_param_stats(optimizer, iteration, path)
    return True


def _train(model, optimizer, lr_scheduler, forward_step, train_dataloader, end_of_epoch_callback, end_of_epoch_callback2, eos_id, indexer=None):
    """train_e2eqa.py:413-552.  `indexer`: an AsyncIndexBuilder when --async-indexer (re-indexing on a side stream; the swap at a step
    boundary replaces the NEW_INDEX_READY / NEW_CHKPT_READY handshake and the reload from disk)."""
    args = get_args()
    model.train()
    guard = None
    sel = [int(v) for v in str(getattr(args, "selective_retention_layers", "0,0,0")).split(",")] + [0, 0, 0]
    keep = int(getattr(args, "recompute_keep_last_layers", 0) or 0)
    micro = int(getattr(args, "question_micro_batches", 1) or 1)
    if keep or any(sel[:3]) or micro > 1:
        from emdr2_amd.training import RetentionGuard
        retr = getattr(model, "evidence_retriever", None)

        def set_micro(m):                             # _cross_entropy_forward_step reads the flag: a finer split after an allocation failure
            args.question_micro_batches = m           # takes effect in the re-run of the very step that failed
        guard = RetentionGuard(model, optimizer, keep=keep, reader=sel[0], context=sel[1], query=sel[2],
                               forward_progress=(lambda: getattr(retr, "searches", 0)) if retr is not None else None, log=print_rank_0,
                               micro=micro, batch=args.batch_size, on_micro_change=set_micro)
    snapshots = None
    if indexer is not None and getattr(args, "save_index_snapshot", False) and args.save:
        # --save-index-snapshot: the index just committed goes to <save>/evidence_index.flat, a chunk per step boundary, paced to cover the
        # shard in half a reload interval (data/index_snapshot.py)
        from emdr2_amd.data.index_snapshot import SNAPSHOT_NAME, IndexSnapshotWriter
        lo, hi = indexer.index.local_rows()
        snapshots = indexer.snapshot_writer = IndexSnapshotWriter(
            indexer.index, chunk_rows=IndexSnapshotWriter.paced_chunk_rows(hi - lo, args.index_reload_interval), log=print_rank_0,
            track_deltas=bool(getattr(args, "save_index_deltas", False)))
        snapshot_path = os.path.join(args.save, SNAPSHOT_NAME)
    # --save-index-deltas: the index whose changed rows follow every checkpoint save but the one an index update takes -- there the next
    # snapshot has just been begun.  (A swap refresher replaces whole images and the live one does not change between swaps: there is
    # nothing for a delta to hold.)
    deltas = None
    if getattr(args, "save_index_deltas", False) and args.save and (indexer.in_place if indexer is not None else getattr(args, "index_writeback", False)):
        from emdr2_amd.data.index_snapshot import SNAPSHOT_NAME
        deltas = indexer.index if indexer is not None else getattr(getattr(model, "evidence_retriever", None), "mips_index", None)
        snapshot_path = os.path.join(args.save, SNAPSHOT_NAME)

    def checkpoint(iteration, finish=False):
        _save(iteration, model, optimizer, lr_scheduler)
        if finish and snapshots is not None and deltas is not None:
            # (a no-op when none is open.)  Before the delta: publishing a snapshot drops the delta of the one it replaces, and a delta
            # against the snapshot just finished brings the chunks it exported steps ago up to this boundary
            snapshots.finish()
        if deltas is not None:
            # after this boundary's writers (refresher rows, write-back) and the snapshot writer's pump, before the next step
            save_index_delta(deltas, snapshot_path, iteration, take_base=indexer is None)
    audit_interval = int(getattr(args, "audit_index_interval", 0) or 0)
    audited = getattr(getattr(model, "evidence_retriever", None), "mips_index", None) if audit_interval > 0 else None
    if audited is not None:
        audit_index(audited, args.iteration)          # what was loaded or restored, before the first step searches it
    state_audit_interval = int(getattr(args, "audit_optimizer_state_interval", 0) or 0)
    if state_audit_interval > 0:
        audit_optimizer_state(optimizer, args.iteration)          # what was initialised or loaded, before the first step runs on it
    param_stats_interval = int(getattr(args, "log_param_stats_interval", 0) or 0)
    stamped = getattr(getattr(model, "evidence_retriever", None), "mips_index", None) if getattr(args, "index_generations", False) else None
    newest_wins = bool(getattr(args, "index_newest_wins", False))
    hit_tracker = getattr(model, "answer_hits", None)        # --retrieval-answer-hits
    read_meter = getattr(model, "reader_mass", None)         # --reader-attention-mass
    start_epoch = args.iteration // args.train_iters_per_epoch
    start_iteration = args.iteration % args.train_iters_per_epoch
    iteration = args.iteration
    sums, t_last = {}, time.time()
    # --skip-nonfinite-steps: the verdict of every step stays on the device (FlatAdam.last_step_skipped); the host learns the counts once
    # per --log-interval (FlatAdam.guard_report)
    skip_guard = optimizer if getattr(optimizer, "skip_nonfinite", False) else None
    max_skips = int(getattr(args, "max_consecutive_skipped_steps", 0) or 0)
    if skip_guard is not None:
        nan_steps = torch.zeros((), dtype=torch.int64, device="cuda")
        skipped_logged = skip_guard.guard_report(clear=False)["skipped_total"]
    for epoch in range(start_epoch, args.epochs):
        print_rank_0('working on epoch {} ...'.format(epoch + 1))
        train_dataloader.sampler.set_epoch(args.seed + epoch)
        for iteration_, batch in enumerate(train_dataloader):
            if iteration_ < start_iteration:
                continue
            start_iteration = 0
            if indexer is not None:
                indexer.pump()
            losses = train_step(forward_step, batch, model, optimizer, lr_scheduler, eos_id, guard=guard)
            iteration += 1
            if state_audit_interval > 0:
                # right behind the step, before any checkpoint save of this boundary: a state that fails is never saved
                maybe_audit_optimizer_state(optimizer, iteration, state_audit_interval)
            if param_stats_interval > 0:
                # behind the step and the audit, while the buckets still hold this step's gradient (until the next zero_grad())
                maybe_log_param_stats(optimizer, iteration, param_stats_interval, getattr(args, "param_stats_file", None))
            if hit_tracker is not None:
                hit_tracker.commit()
            if read_meter is not None:
                read_meter.commit()
            retrieved_ages = None
            if stamped is not None and iteration % args.log_interval == 0 and stamped.last_search_rows is not None:
                # the ages of the rows this step's search returned (the merged rows of all ranks' questions: the same list on every rank),
                # as the search found them: before this boundary's writers, against the weights the forward ran with
                retrieved_ages = stamped.generation_stats(iteration - 1, stamped.last_search_rows)
            if indexer is not None and indexer.maybe_swap(iteration):
                print_rank_0("Training Group: MIPS Index Updated at iteration {}".format(iteration))
                if args.save:
                    _save(iteration, model, optimizer, lr_scheduler)                          # the reference checkpoints at every reload
                if snapshots is not None:
                    if snapshots.active:        # (rolling mode; before a swap, maybe_swap has finished it)
                        print_rank_0("Training Group: finishing the open index snapshot before the next at iteration {}".format(iteration))
                        snapshots.finish()
                    snapshots.begin(snapshot_path, {"iteration": iteration, "refreshes": indexer.refreshes,
                                                    "mode": "rolling" if indexer.in_place else "swap"})
            if getattr(args, "index_writeback", False):
                # after the refresher's rows of this boundary (they come from an older snapshot of the weights): the write-back goes last and
                # wins.  That settles ONE boundary.  Across boundaries nothing orders the two writers -- the refresher's pass reaches a
                # written-back row tens of steps later, with weights up to a pass older -- unless --index-newest-wins: the write-back stamps
                # iteration - 1, the weights the forward ran with, the refresher the step count of its snapshot, and either leaves a row with
                # a higher stamp alone
                skipped = skip_guard.last_step_skipped if skip_guard is not None else None
                if stamped is not None:
                    index_writeback(model, args.batch_size, args.topk_retrievals, generation=writeback_generation(iteration),
                                    newest_wins=newest_wins, skipped=skipped)
                else:
                    index_writeback(model, args.batch_size, args.topk_retrievals, skipped=skipped)
            if retrieved_ages is not None:
                index_generation_line(stamped, iteration, retrieved_ages)
            if audited is not None:
                # after everything that writes the live image at this boundary, before the snapshot writer exports from it
                maybe_audit_index(audited, iteration, audit_interval)
            if snapshots is not None:
                snapshots.pump()
                snapshots.maybe_finalize(iteration)
            if skip_guard is not None:
                # training.py:240-315: a skipped step's losses stay out of the averages, and it counts as a "nan iteration" when their sum
                # is itself non-finite -- here without asking the device for the verdict
                skipped = skip_guard.last_step_skipped
                vals = {k: torch.as_tensor(v, dtype=torch.float32, device=skipped.device) for k, v in losses.items()}
                nan_steps += skipped & ~torch.isfinite(sum(v.sum() for v in vals.values()))
                losses = {k: torch.where(skipped, torch.zeros_like(v), v) for k, v in vals.items()}
            for k, v in losses.items():
                sums[k] = sums.get(k, 0.0) + v
            if iteration % args.log_interval == 0:
                dt = (time.time() - t_last) * 1000.0 / args.log_interval
                t_last = time.time()
                msg = ' iteration {:8d}/{:8d} | elapsed time per iteration (ms): {:.1f} | learning rate: {:.3E} |'.format(
                    iteration, args.train_iters, dt, lr_scheduler.get_lr())
                skipped_now = 0
                if skip_guard is not None:
                    report = skip_guard.guard_report()             # the guard's one host read of the interval
                    skipped_now = report["skipped_total"] - skipped_logged
                    skipped_logged = report["skipped_total"]
                for k in sums:
                    msg += ' {}: {:.6E} |'.format(k, interval_average(float(sums[k]), args.log_interval, skipped_now))
                if skip_guard is not None:
                    msg += ' number of skipped iterations: {:3d} | number of nan iterations: {:3d} |'.format(skipped_now, int(nan_steps))
                    nan_steps.zero_()
                if hit_tracker is not None:                   # (collective: every rank is here at the same iterations)
                    msg += hit_tracker.line()
                if read_meter is not None:
                    msg += read_meter.line()
                print_rank_0(msg)
                sums = {}
                if skip_guard is not None:
                    if report["step"] is not None:
                        print_rank_0(skipped_step_line(report, iteration - (optimizer.step_count - report["step"])))
                    if 0 < max_skips <= report["longest_run"]:
                        # every rank holds the same counts at the same iterations (FlatAdam: the verdict needs no collective)
                        raise RuntimeError("%d consecutive optimizer steps had non-finite gradients and were skipped "
                                           "(--max-consecutive-skipped-steps %d), seen at iteration %d" % (report["longest_run"], max_skips, iteration))
            if args.save and args.save_interval and iteration % args.save_interval == 0:
                checkpoint(iteration)
            if args.eval_interval and iteration % args.eval_interval == 0 and end_of_epoch_callback is not None:
                end_of_epoch_callback(model, iteration)
                end_of_epoch_callback2(model, iteration)
            if args.exit_interval and iteration % args.exit_interval == 0:                    # train_e2eqa.py:526-540
                print_rank_0('exiting the program at iteration {}'.format(iteration))
                if args.save:
                    checkpoint(iteration, finish=True)
                if snapshots is not None:
                    snapshots.finish()
                return iteration
        if args.save:
            checkpoint(iteration, finish=True)
        if snapshots is not None:
            snapshots.finish()                        # (a no-op when none is open)
        if end_of_epoch_callback is not None:
            end_of_epoch_callback(model, epoch + 1)
            end_of_epoch_callback2(model, epoch + 1)
    return iteration


def train(train_valid_datasets_provider, model_provider, forward_step=_cross_entropy_forward_step, end_of_epoch_callback_provider=None,
          end_of_training_callback_provider=None, eos_id=None, indexer_provider=None):
    """train_e2eqa.py:555-621."""
    args = get_args()
    train_dataloader = None
    if args.epochs > 0:
        train_dataset, valid_dataset = train_valid_datasets_provider()
        train_dataloader = build_data_loader(train_dataset, args.batch_size, args.num_workers, drop_last=not args.keep_last)
        args.train_iters_per_epoch = len(train_dataloader)
        args.train_iters = args.epochs * args.train_iters_per_epoch
    else:
        args.train_iters_per_epoch, args.train_iters = 1, 0
    cb1 = cb2 = None
    if args.epochs > 0 and end_of_epoch_callback_provider is not None:
        cb1, cb2 = end_of_epoch_callback_provider(args.valid_data), end_of_epoch_callback_provider(args.test_data)
    model, optimizer, lr_scheduler = setup_model_and_optimizer(model_provider)
    if args.iteration == 0 and args.pretrained_checkpoint is not None:                     # train_e2eqa.py:586-593: weights only
        checkpointing.load_checkpoint(args.pretrained_checkpoint, model, None, None)
    print_rank_0('done with setups ...')
    print_rank_0('training ...')
    if args.epochs > 0 and args.emdr2_training:
        indexer = indexer_provider(model) if (indexer_provider is not None and args.async_indexer) else None
        _train(model, optimizer, lr_scheduler, forward_step, train_dataloader, cb1, cb2, eos_id, indexer)
    results = {}
    if end_of_training_callback_provider is not None:
        for name, path in (("validation", args.valid_data), ("test", args.test_data)):
            if path:
                results[name] = end_of_training_callback_provider(path)(model, epoch=-1)
    print_rank_0('done :-)')
    return model, results
