"""Command-line flags of the QA task: the flag set of examples/openqa/emdr2_{nq,trivia,webq}.sh with the reference's names, types and
defaults (megatron/arguments.py:24-596, tasks/run.py:24-67), so those scripts run against this package unchanged.  Flags that configure
machinery this build replaces are accepted and recorded but have no effect: --fp16 (announced at start-up as bf16 activations + fp32
masters, no loss scaling: args.params_dtype), --DDP-impl, --distributed-backend, --num-workers, --faiss-use-gpu (the index always lives in HBM), --max-training-rank /
--async-indexer's extra GPU group (re-indexing runs on a side stream of the trainers), --stale-checkpoint-path, --mmap-warmup.
Unknown flags raise, like argparse in the reference."""
import argparse
import os


def get_parser():
    p = argparse.ArgumentParser(description='EMDR2 on MI355X', allow_abbrev=False)
    g = p.add_argument_group('network size')
    g.add_argument('--num-layers', type=int, default=None)
    g.add_argument('--hidden-size', type=int, default=None)
    g.add_argument('--num-attention-heads', type=int, default=None)
    g.add_argument('--kv-channels', type=int, default=None)
    g.add_argument('--ffn-hidden-size', type=int, default=None)
    g.add_argument('--max-position-embeddings', type=int, default=None)
    g.add_argument('--make-vocab-size-divisible-by', type=int, default=128)
    g.add_argument('--layernorm-epsilon', type=float, default=1e-5)
    g = p.add_argument_group('regularization')
    g.add_argument('--attention-dropout', type=float, default=0.1)
    g.add_argument('--hidden-dropout', type=float, default=0.1)
    g.add_argument('--weight-decay', type=float, default=0.01)
    g.add_argument('--clip-grad', type=float, default=1.0)
    g = p.add_argument_group('training')
    g.add_argument('--batch-size', type=int, default=None)
    g.add_argument('--checkpoint-activations', action='store_true')
    g.add_argument('--recompute-keep-last-layers', type=int, default=0,
                   help='(not in the reference) with --checkpoint-activations: keep the activations of the last N reader-encoder layers '
                        'instead of re-running them in the backward (~33 GB of HBM per layer at batch 64 x top-k 50 x 512 tokens)')
    g.add_argument('--selective-retention-layers', type=str, default='0,0,0',
                   help='(not in the reference) with --checkpoint-activations: READER,CONTEXT,QUERY encoder layers that keep 6 of their ~16 '
                        '[tokens, h] activation tensors and rebuild the rest (both LayerNorm outputs, the FFN pre-activation and GELU output) in '
                        'the backward, instead of being re-run whole (+6.3 GB per reader-encoder layer, +3.0 GB per context-tower layer at '
                        'batch 64 x top-k 50; packed row counts keep growing by 16,384-row steps over the first tens of steps: leave ~25 GB free)')
    g.add_argument('--question-micro-batches', type=int, default=1,
                   help='(not in the reference) run the forward / backward of a step over the batch in M groups of questions '
                        '(EMDR2Model.forward_backward: one MIPS search for the whole batch, everything after it per group, gradients summed in '
                        'the fp32 buckets, losses with batch-wide denominators).  M > 1 keeps every activation of a group instead of re-running '
                        'layers in the backward: --checkpoint-activations is then ignored (batch 64 x top-k 50: M = 4, top-k 100: M = 8)')
    g.add_argument('--seed', type=int, default=1234)
    g.add_argument('--init-method-std', type=float, default=0.02)
    g.add_argument('--lr', type=float, default=None)
    g.add_argument('--lr-decay-style', type=str, default='linear', choices=['linear'])
    g.add_argument('--lr-decay-iters', type=int, default=None)
    g.add_argument('--min-lr', type=float, default=0.0)
    g.add_argument('--warmup', type=float, default=0.01)
    g.add_argument('--log-interval', type=int, default=100)
    g.add_argument('--fp16', action='store_true')
    g.add_argument('--fp32-validation', action='store_true',
                   help='VALIDATION ONLY: run the model in fp32 on the fp32 matrix cores (the reference\'s arithmetic when --fp16 is not given, '
                        'megatron/training.py:55-56): slow, dense layouts, dropout must be 0 -- exists so that "logits within 1e-3 fp32" can be tested')
    g.add_argument('--model-parallel-size', type=int, default=1)
    g.add_argument('--distributed-backend', default='nccl')
    g.add_argument('--DDP-impl', default='local')
    g.add_argument('--local_rank', type=int, default=None)
    g.add_argument('--num-workers', type=int, default=2)
    g = p.add_argument_group('checkpointing')
    g.add_argument('--save', type=str, default=None)
    g.add_argument('--save-interval', type=int, default=None)
    g.add_argument('--load', type=str, default=None)
    g.add_argument('--no-save-optim', action='store_true')
    g.add_argument('--no-load-optim', action='store_true')
    g.add_argument('--pretrained-checkpoint', type=str, default=None)
    g.add_argument('--ict-load', type=str, default=None)
    g.add_argument('--exit-interval', type=int, default=None)
    g.add_argument('--pretrained-t5-load', type=str, default=None)
    g.add_argument('--pretrained-dpr-load', type=str, default=None)
    g.add_argument('--stale-checkpoint-path', type=str, default=None)
    g = p.add_argument_group('validation')
    g.add_argument('--eval-interval', type=int, default=1000)
    g.add_argument('--eval-iters', type=int, default=100)
    g.add_argument('--eval-batch-size', type=int, default=None)
    g.add_argument('--beam-size', type=int, default=1)
    g.add_argument('--max-decode-len', type=int, default=512)
    g = p.add_argument_group('data')
    g.add_argument('--seq-length', type=int, default=None)
    g.add_argument('--seq-length-ret', type=int, default=256)
    g.add_argument('--decoder-seq-length', type=int, default=None)
    g.add_argument('--vocab-file', type=str, default=None)
    g.add_argument('--vocab-extra-ids', type=int, default=0)
    g.add_argument('--tokenizer-type', type=str, default=None, choices=['BertWordPieceLowerCase', 'BertWordPieceCase'])
    g.add_argument('--data-impl', type=str, default='infer', choices=['mmap', 'infer'])
    g.add_argument('--mmap-warmup', action='store_true')
    g.add_argument('--evidence-data-path', type=str, default=None)
    g.add_argument('--indexed-evidence-data-path', type=str, default=None)
    g.add_argument('--indexed-title-data-path', type=str, default=None)
    g.add_argument('--embedding-path', type=str, default=None)
    g.add_argument('--sample-rate', type=float, default=1.0)
    g = p.add_argument_group('task (tasks/run.py)')
    g.add_argument('--task', type=str, required=True)
    g.add_argument('--epochs', type=int, default=None)
    g.add_argument('--keep-last', action='store_true')
    g.add_argument('--train-data', nargs='+', default=None)
    g.add_argument('--valid-data', nargs='*', default=None)
    g.add_argument('--test-data', nargs='*', default=None)
    g = p.add_argument_group('emdr2')
    g.add_argument('--topk-retrievals', type=int, default=100)
    g.add_argument('--emdr2-training', action='store_true')
    g.add_argument('--retriever-score-scaling', action='store_true')
    g.add_argument('--update-retriever', action='store_true')
    g.add_argument('--ret-kldiv', action='store_true')
    g.add_argument('--allow-trivial-doc', action='store_true')
    g.add_argument('--disable-retriever-dropout', action='store_true')
    g.add_argument('--no-query-embedder-training', action='store_true')
    g.add_argument('--no-context-embedder-training', action='store_true')
    g.add_argument('--faiss-use-gpu', action='store_true')
    g.add_argument('--max-training-rank', type=int, default=None)
    g.add_argument('--async-indexer', action='store_true')
    g.add_argument('--index-reload-interval', type=int, default=500)
    g.add_argument('--index-refresh-in-place', action='store_true',
                   help='(not in the reference) with --async-indexer: write re-embedded evidence rows into the index image that is being '
                        'searched at every step boundary instead of filling a spare image and swapping it in every --index-reload-interval '
                        'steps.  No spare fp16 image and no spare int8 shadow image: half the index HBM of the swap mode.  A choice of '
                        'semantics, not a tuning knob: searches then see a MIX of two embedding generations -- rows already re-embedded in '
                        'the current pass next to rows of the pass before -- where the default, the reference\'s update_index, replaces '
                        'the whole index atomically.  The refresher writes whatever its pass reaches, also over rows that '
                        '--index-writeback has written from newer weights since; --index-newest-wins changes that')
    g.add_argument('--index-writeback', action='store_true',
                   help='(not in the reference; needs --disable-retriever-dropout) at every step boundary write the embeddings the step has '
                        'just computed with the LIVE context encoder for the batch-size x topk passages it retrieved into the index rows they '
                        'were retrieved from (with several ranks: two all-gathers per step, every rank updates its own shard).  No encoder '
                        'work is added.  A row holds whatever was written LAST: a passage retrieved by several questions keeps the last '
                        'one\'s embedding, and the rolling refresher (--async-indexer --index-refresh-in-place) will later overwrite a '
                        'written-back row with its older snapshot\'s embedding when its pass comes round (unless --index-newest-wins is '
                        'given, which makes every in-place writer leave rows from newer weights alone).  A choice of semantics, not a '
                        'tuning knob: the index holds a mix of embedding generations, the retrieved rows being the freshest.  Allowed '
                        'without --async-indexer; with --async-indexer it needs --index-refresh-in-place (in swap mode every write would '
                        'be discarded at the next swap)')
    g.add_argument('--index-generations', action='store_true',
                   help='(not in the reference) the evidence index keeps one 32-bit generation stamp per row on the device (84 MB at 21 M '
                        'rows): the number of optimizer steps the weights that wrote the row had taken -- 0 for rows loaded from '
                        '--embedding-path; rows restored from an index snapshot get the stamps the snapshot saved with them '
                        '(--save-index-snapshot), or, from a snapshot without stamps, its iteration -- ages are then a lower bound.  '
                        'Every writer stamps what it writes.  At every --log-interval rank 0 prints one '
                        'line: mean / max age, in steps, of the rows the last step retrieved (as its search found them), mean / max age of '
                        'the whole index, and the rows that newest-wins updates have left alone since the last line.  One small device pass '
                        'and two small all-reduces per statistic, at iterations that depend on --log-interval alone.  No search result changes')
    g.add_argument('--index-newest-wins', action='store_true',
                   help='(not in the reference; implies --index-generations; needs an in-place writer: --index-refresh-in-place or '
                        '--index-writeback) the rolling refresher and the write-back leave a row alone when its stamp is above the '
                        'generation they would write: a row written back from the weights of step t - 1 is no longer replaced by the '
                        'refresher\'s embedding from a snapshot taken up to a whole pass earlier.  Ties write, so within one generation the '
                        'last writer still wins.  A choice of semantics, not a tuning knob: without it a row holds whatever was written '
                        'LAST, with it whatever came from the NEWEST weights; the index is a fresh build of its rows either way')
    g.add_argument('--index-refresh-oldest-first', action='store_true',
                   help='(not in the reference; implies --index-generations; needs --async-indexer --index-refresh-in-place) the rolling '
                        'refresher embeds, at every step, the OLDEST rows of its shard that are older than its weight snapshot -- chosen on '
                        'the device from the generation stamps, lowest rows first among equal stamps -- instead of the next rows in row '
                        'order.  No encoder forward is spent on a row that --index-writeback has stamped since the snapshot (which '
                        '--index-newest-wins would refuse to overwrite anyway), and a pass ends as soon as no row is older than its '
                        'snapshot instead of after a fixed count.  The pace (rows per step) is unchanged.  On an index with uniform '
                        'stamps -- a fresh start, a resume from a snapshot without stamps -- the order is the row order.  Rank 0 prints '
                        'one line per completed pass')
    g.add_argument('--context-embeddings-from-index', action='store_true',
                   help='(not in the reference; needs --no-context-embedder-training) take the embeddings of the batch-size x topk retrieved '
                        'passages from the index rows the search returned instead of running the frozen context encoder over them, in '
                        'training and in evaluation mode: one gather launch (with several ranks plus one all-reduce of the gathered buffer) '
                        'replaces the context tower\'s forward.  A choice of semantics, not a tuning knob: the prior is computed from '
                        'WHATEVER the index holds -- fp16 rows widened exactly to fp32, no dropout.  For an index built from the frozen '
                        'context encoder that is the tower\'s own output to within its bf16 arithmetic; an index built from other weights '
                        'gives other scores.  Refused with --index-writeback (the step no longer computes anything to write back).  '
                        '--async-indexer, with or without --index-refresh-in-place, stays allowed: re-embedding with a frozen encoder '
                        'rewrites equal rows, and rows are read from the live image on the main stream, in the same order as the search')
    g.add_argument('--save-index-snapshot', action='store_true',
                   help='(not in the reference; needs --save) with --async-indexer: after every index update write the index just committed '
                        'to the one file <save>/evidence_index.flat (+ .meta), overwritten atomically like the reference\'s embedding file, a '
                        'chunk per step; with --load, start from <load>/evidence_index.flat when its meta is valid, fits the evidence and is '
                        'not newer than the checkpoint, else from --embedding-path as without the flag.  Swap mode: the live index does not '
                        'change between swaps, so a resumed run searches exactly what the uninterrupted run searched at that step; the '
                        'refresher\'s in-flight pass is not saved and restarts.  With --index-refresh-in-place the snapshot is a mix of '
                        'embedding generations, as the live index is, and the pass cursor is not saved')
    g.add_argument('--save-index-deltas', action='store_true',
                   help='(not in the reference; needs --save-index-snapshot) incremental snapshots: the snapshot writer also keeps a 64-bit '
                        'key per exported row, and every checkpoint save that is not itself an index update is followed by '
                        '<save>/evidence_index.flat.delta (+ .delta.meta): the rows whose key differs from the published snapshot\'s, '
                        'found on the device in one pass over the live image at the step boundary, after the refresher\'s rows and the '
                        'write-back.  The delta is cumulative (always relative to the published snapshot, one file, overwritten '
                        'atomically) and is dropped when a new snapshot is published.  With --index-writeback and no --async-indexer one '
                        'synchronous snapshot is taken at the first checkpoint save.  With --load, the snapshot plus a delta that is not '
                        'newer than the checkpoint is the index the checkpointed run was searching.  Rank 0 prints one line per delta')
    g.add_argument('--audit-index-interval', type=int, default=0,
                   help='(not in the reference) N > 0: audit the evidence index in HBM (DistributedBruteForceIndex.audit: the premises of '
                        'the search\'s exactness proof and the "byte for byte a fresh build" contract, one streaming pass over the live '
                        'images) once before the first step and at every iteration divisible by N, at the step boundary after the index '
                        'swap and the write-back and before the snapshot writer reads the image.  Rank 0 prints one line per audit; a '
                        'failing audit raises RuntimeError on every rank.  Two small all-reduces per audit when the index is sharded, at '
                        'iterations that depend on N alone.  0: off, nothing changes')
    g.add_argument('--indexer-batch-size', type=int, default=128)
    g.add_argument('--indexer-log-interval', type=int, default=1000)
    g.add_argument('--report-topk-accuracies', nargs='+', type=int, default=[])
    g.add_argument('--retrieval-answer-hits', action='store_true',
                   help='(not in the reference, which measures this in a separate evaluator over the evidence text: '
                        'tasks/openqa/dense_retriever/evaluation) report how often, and at which rank, the passages the reader is shown hold a '
                        'reference answer, matched on the device against the token ids of the evidence arena (include/emdr2_answers.h: one '
                        'launch pair per training step and per evaluation batch).  Training: every --log-interval line gains '
                        '"answer hits@k" for the questions since the last line (data-parallel ranks summed) and "hit mass", the retriever\'s '
                        'probability mass on answer-bearing passages.  Evaluation: "Answer Hits@k" beside the exact match score.  k: '
                        '--report-topk-accuracies cut to --topk-retrievals (1 5 20 and --topk-retrievals when none are given).  Off: no '
                        'launch, no output changes')
    g.add_argument('--reader-attention-mass', action='store_true',
                   help='(not in the reference) report which retrieved passages the FiD decoder READS: the cross-attention probability mass per '
                        'passage slot, summed over decoder layers, heads and answer positions and normalised per question (csrc/attention_mass.hip: '
                        'one small launch behind each decoder cross-attention forward).  Training: every --log-interval line gains "read entropy" '
                        '(mean entropy of that distribution) and "read-prior agree" (questions whose most-read passage is the retriever\'s top '
                        'one); with --retrieval-answer-hits also "read mass" (mass on answer-bearing passages, comparable to "hit mass") and '
                        '"read top1 hit"; the evaluation then prints "Read Top-1 Hit".  Needs 64-channel heads; not with --fp32-validation.  '
                        'Off: no launch, no output changes')
    g.add_argument('--retriever-distill-attention', action='store_true',
                   help='(not in the reference) train the retriever towards what the reader READS (FiD-KD): the retriever loss is '
                        'KL(read || prior) per question, where "read" is the FiD decoder\'s cross-attention probability mass per passage slot -- '
                        'the quantity of --reader-attention-mass, measured in the FiD pass the step runs anyway and taken as a constant.  A '
                        'choice of objective, not a tuning knob: it replaces the EMDR2 marginal, and the no-grad one-context pass over all '
                        'B x K passages that only the marginal (and --ret-kldiv) needs is not run.  Needs --update-retriever and 64-channel '
                        'heads; exclusive with --ret-kldiv; not with --fp32-validation.  Off: the step launches what it launched before')
    g.add_argument('--attention-mass-value-norms', action='store_true',
                   help='(not in the reference) weight every attention probability of the mass by the norm of its key\'s value vector, '
                        '||v_j||_2 per head and layer (ATLAS-style attention distillation; csrc/attention_mass.hip: one norm launch per '
                        'decoder layer and group, once per batch under greedy decoding).  A choice of what "read" means, wherever the mass is '
                        'collected: the log fields of --reader-attention-mass and the target of --retriever-distill-attention change together.  '
                        'Needs one of those two flags')
    g.add_argument('--deterministic-gradients', action='store_true',
                   help='(not in the reference) bit-reproducible parameter gradients: the weight-gradient GEMMs, the LayerNorm gain / bias '
                        'gradients and the embedding backward sum in a fixed order through a workspace (the *_ordered entries of '
                        'include/emdr2_ops.h) instead of fp32 atomics, so the same step from the same state gives the same bits.  Not '
                        'promised: equality with a run without the flag, across world sizes or across shapes that choose another split.  '
                        'Not with --fp32-validation.  Off: every launch is what it was')
    g.add_argument('--skip-nonfinite-steps', action='store_true',
                   help='(the reference: FP16_Optimizer skips a step on overflow, fp16/fp16.py:420-474, training.py:223-228) a step whose global '
                        'gradient norm is NaN or Inf changes no weight, moment or working copy: decided and applied on the device (one '
                        'small launch per step, no host read), the same on every data-parallel replica.  The iteration, the optimizer '
                        'step count, the dropout step and the learning-rate schedule advance all the same.  The log line gains "number of '
                        'skipped iterations" and "number of nan iterations", skipped steps stay out of the loss averages, and '
                        '--index-writeback writes no row of a skipped step and no non-finite row.  Not with --fp32-validation.  Off: '
                        'every launch is what it was')
    g.add_argument('--max-consecutive-skipped-steps', type=int, default=0,
                   help='with --skip-nonfinite-steps: end the run (RuntimeError on every rank, at a --log-interval boundary) once this many '
                        'consecutive steps were skipped.  0: no limit')
    g.add_argument('--audit-optimizer-state-interval', type=int, default=0,
                   help='(not in the reference; Megatron-LM: --check-weight-hash-across-dp-replicas-interval) audit the optimizer state '
                        'before the first step and at every iteration divisible by N, at the step boundary before that boundary\'s '
                        'checkpoint: one streaming HIP pass per bucket (csrc/state_audit.hip) over the fp32 masters, both Adam moments and '
                        'the bf16 working copies counts non-finite elements, negative second moments and working copies that are not the '
                        'rounding of their master, and digests the bit patterns; two small all-reduces compare the digests of the '
                        'data-parallel replicas.  Rank 0 prints one line; an unsound state or a replica that differs raises RuntimeError on '
                        'every rank, naming the array, the parameter and the element.  Checkpoints gain a digest that the next load '
                        'verifies.  Promised: equal bits and the invariants, not right values.  Not with --fp32-validation.  0: never, '
                        'every launch, log line and checkpoint byte is what it was')
    g.add_argument('--log-param-stats-interval', type=int, default=0,
                   help='(not in the reference; Megatron-LM: --log-params-norm, --log-num-zeros-in-grad) at every iteration divisible by N, '
                        'right behind the step: per-parameter statistics of the optimizer buckets from one streaming HIP pass per bucket '
                        '(csrc/param_stats.hip) over gradients, fp32 masters and both Adam moments, one host read.  Rank 0 prints a '
                        'summary line (grad norm, params norm, num zeros, the clip factor, the five parameters with the largest '
                        'lr * |d| / |w| and the five with the largest share of the squared gradient norm) and one line per group '
                        '(a layer, or the first two name components).  The sums are added in a fixed order: replicas hold the same bits '
                        'with no collective.  Not with --fp32-validation.  0: never, no launch, no buffer, every log line is what it was')
    g.add_argument('--param-stats-file', type=str, default=None,
                   help='with --log-param-stats-interval: rank 0 appends one JSON line per call with every parameter\'s record')
    return p


def parse_args(argv=None):
    args = get_parser().parse_args(argv)
    args.rank = int(os.getenv('RANK', '0'))
    args.world_size = int(os.getenv('WORLD_SIZE', '1'))
    if args.local_rank is None:
        args.local_rank = int(os.getenv('LOCAL_RANK', '0'))
    if args.model_parallel_size != 1:
        raise NotImplementedError("tensor model parallelism is 1 on this path (the reference asserts the same, dualencoder_model.py:15)")
    for name in ('num_layers', 'hidden_size', 'num_attention_heads', 'max_position_embeddings', 'seq_length', 'decoder_seq_length', 'batch_size', 'lr'):
        if getattr(args, name) is None:
            raise ValueError("--%s is required" % name.replace('_', '-'))
    if args.ffn_hidden_size is None:
        args.ffn_hidden_size = 4 * args.hidden_size                       # arguments.py:90-91
    if args.kv_channels is None:
        args.kv_channels = args.hidden_size // args.num_attention_heads
    if args.kv_channels * args.num_attention_heads != args.hidden_size:
        raise ValueError("kv-channels * num-attention-heads must equal hidden-size")
    if args.eval_batch_size is None:
        args.eval_batch_size = args.batch_size
    if args.load and args.ict_load:
        raise ValueError("--load and --ict-load are exclusive (indexer_emdr2.py:47)")
    if args.save_index_snapshot and not args.save:
        raise ValueError("--save-index-snapshot needs --save (the snapshot lives next to the checkpoints)")
    if args.save_index_deltas and not args.save_index_snapshot:
        raise ValueError("--save-index-deltas needs --save-index-snapshot (a delta is relative to the published snapshot)")
    if args.index_writeback and not args.disable_retriever_dropout:
        raise ValueError("--index-writeback needs --disable-retriever-dropout (a training-mode context tower would write dropout noise into the index)")
    if args.index_writeback and args.async_indexer and not args.index_refresh_in_place:
        raise ValueError("--index-writeback with --async-indexer needs --index-refresh-in-place (in swap mode a refresh is always in progress: "
                         "the index refuses in-place updates, and the next swap would discard them anyway)")
    if args.index_newest_wins:
        if not (args.index_writeback or (args.async_indexer and args.index_refresh_in_place)):
            raise ValueError("--index-newest-wins needs an in-place writer of the index: --index-writeback or --async-indexer "
                             "--index-refresh-in-place (the swap refresher replaces whole images: there is nothing to arbitrate)")
        args.index_generations = True
    if args.index_refresh_oldest_first:
        if not (args.async_indexer and args.index_refresh_in_place):
            raise ValueError("--index-refresh-oldest-first needs the rolling refresher: --async-indexer --index-refresh-in-place (the swap "
                             "refresher rebuilds whole images: there is no order to choose)")
        args.index_generations = True
    if args.audit_index_interval < 0:
        raise ValueError("--audit-index-interval must be >= 0")
    if args.reader_attention_mass and (args.kv_channels != 64 or args.fp32_validation):
        # (the model build refuses the same: emdr2_model.check_reader_attention_mass)
        raise ValueError("--reader-attention-mass reads the fused bf16 attention kernels' operands and statistics: it needs --kv-channels 64 "
                         "and does not run with --fp32-validation")
    if args.retriever_distill_attention:
        if not args.update_retriever:
            raise ValueError("--retriever-distill-attention is a retriever loss: it needs --update-retriever")
        if args.ret_kldiv:
            raise ValueError("--retriever-distill-attention and --ret-kldiv are exclusive (each names THE retriever loss)")
        if args.kv_channels != 64 or args.fp32_validation:
            raise ValueError("--retriever-distill-attention distils from the attention mass, which reads the fused bf16 attention kernels' "
                             "operands and statistics: it needs --kv-channels 64 and does not run with --fp32-validation")
    if args.attention_mass_value_norms and not (args.reader_attention_mass or args.retriever_distill_attention):
        raise ValueError("--attention-mass-value-norms changes what the attention mass holds: it needs --reader-attention-mass or "
                         "--retriever-distill-attention, which collect it")
    if args.deterministic_gradients and args.fp32_validation:
        raise ValueError("--deterministic-gradients orders the sums of the bf16 training path: it does not run with --fp32-validation "
                         "(the fp32 validation kernels keep their atomics)")
    if args.skip_nonfinite_steps and args.fp32_validation:
        raise ValueError("--skip-nonfinite-steps guards the optimizer step of the bf16 training path: it does not run with --fp32-validation")
    if args.max_consecutive_skipped_steps < 0:
        raise ValueError("--max-consecutive-skipped-steps must be >= 0")
    if args.max_consecutive_skipped_steps and not args.skip_nonfinite_steps:
        raise ValueError("--max-consecutive-skipped-steps needs --skip-nonfinite-steps (nothing is skipped without it)")
    if args.audit_optimizer_state_interval < 0:
        raise ValueError("--audit-optimizer-state-interval must be >= 0")
    if args.audit_optimizer_state_interval and args.fp32_validation:
        raise ValueError("--audit-optimizer-state-interval audits the buckets of the bf16 training path (fp32 masters against their bf16 working "
                         "copies): it does not run with --fp32-validation")
    if args.log_param_stats_interval < 0:
        raise ValueError("--log-param-stats-interval must be >= 0")
    if args.log_param_stats_interval and args.fp32_validation:
        raise ValueError("--log-param-stats-interval reads the flat buckets of the bf16 training path: it does not run with --fp32-validation")
    if args.param_stats_file and not args.log_param_stats_interval:
        raise ValueError("--param-stats-file needs --log-param-stats-interval (nothing is collected without it)")
    if args.context_embeddings_from_index and not args.no_context_embedder_training:
        raise ValueError("--context-embeddings-from-index needs --no-context-embedder-training (the context tower is not run, so it would "
                         "silently stop receiving gradients)")
    if args.context_embeddings_from_index and args.index_writeback:
        raise ValueError("--context-embeddings-from-index and --index-writeback are exclusive (the step reads the passages' embeddings from "
                         "the index: it no longer computes anything to write back)")
    args.iteration = 0
    # the reference's --fp16 (fp16 activations, fp32 masters inside FP16_Optimizer, dynamic loss scaling) maps to this build's ONLY
    # precision mode: bf16 activations and working weights, fp32 master weights and gradients, no loss scaling.  Said once, recorded in args.
    args.compute_dtype = 'fp32' if getattr(args, 'fp32_validation', False) else 'bf16'
    args.params_dtype = args.compute_dtype
    args.master_dtype = 'fp32'
    if args.rank == 0 and args.compute_dtype == 'fp32':
        print("emdr2_amd: --fp32-validation: fp32 activations and weights on the fp32 matrix cores (validation only: slow, dense layouts, no dropout)",
              flush=True)
    elif args.rank == 0:
        print("emdr2_amd: %sbf16 activations / working weights with fp32 master weights and fp32 weight gradients; no loss scaling "
              "(there is no fp16 compute mode in this build; --fp32-validation runs the slow fp32 validation path)"
              % ("--fp16 requested -> " if args.fp16 else ""), flush=True)
    return args
