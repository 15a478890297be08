"""CPU: --context-embeddings-from-index at the parser.  The flag is a choice of semantics that only makes sense over a frozen context
encoder; the two combinations that would silently do something else are refused with a reason."""
import pytest

# the reference script's flag set (tests/test_tasks_cpu.py)
BASE = ("--task OPENQA --num-layers 12 --hidden-size 768 --num-attention-heads 12 --kv-channels 64 --ffn-hidden-size 3072 --model-parallel-size 1 "
        "--train-data a.tsv --valid-data b.tsv --test-data c.tsv --evidence-data-path e --indexed-evidence-data-path x --indexed-title-data-path y "
        "--save-interval 500 --save s --load s --pretrained-t5-load p --pretrained-dpr-load d --stale-checkpoint-path d --embedding-path e "
        "--log-interval 20 --eval-interval 500 --eval-iters 10 --weight-decay 1.0e-1 --seq-length 512 --seq-length-ret 256 --decoder-seq-length 32 "
        "--max-decode-len 32 --max-position-embeddings 512 --fp16 --vocab-file v --num-workers 2 --distributed-backend nccl "
        "--checkpoint-activations --tokenizer-type BertWordPieceLowerCase --epochs 10 --sample-rate 1.0 --batch-size 8 --eval-batch-size 8 "
        "--beam-size 1 --lr 2e-5 --warmup 0.01 --DDP-impl local --lr-decay-style linear --max-training-rank 8 --faiss-use-gpu "
        "--topk-retrievals 50 --emdr2-training --retriever-score-scaling --update-retriever --allow-trivial-doc --async-indexer "
        "--index-reload-interval 500").split()


def test_the_reference_flag_set_parses_with_the_mode_off():
    from emdr2_amd import arguments
    a = arguments.parse_args(BASE)
    assert a.context_embeddings_from_index is False and a.no_context_embedder_training is False


def test_the_flag_is_accepted_over_a_frozen_context_encoder():
    from emdr2_amd import arguments
    a = arguments.parse_args(BASE + ["--no-context-embedder-training", "--context-embeddings-from-index"])
    assert a.context_embeddings_from_index is True and a.no_context_embedder_training is True and a.async_indexer
    # the refresher stays allowed in both of its modes
    a = arguments.parse_args(BASE + ["--no-context-embedder-training", "--context-embeddings-from-index", "--index-refresh-in-place"])
    assert a.context_embeddings_from_index and a.index_refresh_in_place


def test_the_flag_is_refused_while_the_context_encoder_is_trained():
    from emdr2_amd import arguments
    with pytest.raises(ValueError, match="--no-context-embedder-training"):
        arguments.parse_args(BASE + ["--context-embeddings-from-index"])


def test_the_flag_is_refused_together_with_the_write_back():
    from emdr2_amd import arguments
    with pytest.raises(ValueError, match="--index-writeback"):
        arguments.parse_args(BASE + ["--no-context-embedder-training", "--context-embeddings-from-index", "--index-writeback",
                                     "--disable-retriever-dropout", "--index-refresh-in-place"])


def test_the_help_text_states_the_semantics():
    from emdr2_amd import arguments
    text = " ".join(arguments.get_parser().format_help().split())
    assert "--context-embeddings-from-index" in text and "WHATEVER the index holds" in text and "not in the reference" in text
