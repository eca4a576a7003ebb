from .accuracy_calculator import CustomCalculator, get_accuracy_calculator
from .evaluate import evaluate, evaluate_multi_k, evaluate_sharded, get_tester
from .batch_map import build_batch_map_calculator, build_fast_eval_subset, compute_batch_map, make_subset
from .get_knn import get_knn
from .train_step import GradientAverager, backward_step, make_averager, train_step
from . import hamming
from .ndcg import NDCG, ndcg_at, ndcg_from_sums, p_topK
from .radius_metrics import get_precision_recall_by_Hamming_Radius, pr_curve, precision_within_radius, radius_curves

__all__ = ["CustomCalculator", "get_accuracy_calculator", "evaluate", "evaluate_multi_k", "evaluate_sharded", "get_tester",
           "get_knn", "hamming", "radius_curves", "precision_within_radius", "pr_curve", "get_precision_recall_by_Hamming_Radius",
           "NDCG", "ndcg_at", "ndcg_from_sums", "p_topK",
           "build_batch_map_calculator", "compute_batch_map", "build_fast_eval_subset", "make_subset",
           "GradientAverager", "backward_step", "make_averager", "train_step"]
