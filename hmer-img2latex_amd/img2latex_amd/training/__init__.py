"""Training step of the hot path (reference img2latex/training/trainer.py:303-343, fp32 branch)."""
from .constraint import ArgumentTable, BracketTable
from .dp import OverlappedAllReduce, all_reduce_gradients, shard_batch
from .metrics import bleu_n_score, calculate_metrics, levenshtein_distance, masked_accuracy, token_list_accuracy
from .predictor import DetokenizeTable, Predictor, TokenTable, detokenize_table, save_checkpoint, token_image
from .tokenizer import TokenizeTable, pack_texts, tokenize_image, tokenize_table
from .vocab import VocabFit, fit_formulas_file, fit_vocabulary, split_lines
from .train_step import TrainStep
from .distill import Teacher
from .risk import RiskObjective
from .epoch_policy import EarlyStopping, PlateauSchedule
from .validate import BleuSampler, ValidationTimeout, Validator, teacher_forced_eval, validate

__all__ = ["TrainStep", "Teacher", "RiskObjective", "Predictor", "TokenTable", "DetokenizeTable", "detokenize_table", "token_image", "TokenizeTable", "tokenize_table", "tokenize_image", "pack_texts", "fit_vocabulary", "fit_formulas_file", "split_lines", "VocabFit", "save_checkpoint", "all_reduce_gradients", "shard_batch",
           "calculate_metrics", "levenshtein_distance", "bleu_n_score", "masked_accuracy", "token_list_accuracy",
           "Validator", "BleuSampler", "validate", "teacher_forced_eval", "ValidationTimeout", "PlateauSchedule", "EarlyStopping", "BracketTable", "ArgumentTable"]
