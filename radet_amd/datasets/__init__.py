from .bop import DATASETS, BOPDataset, CocoDataset, YcbvDataset, build_dataset
from .dataset_wrappers import ClassBalancedDataset, ConcatDataset, MixDataset, RepeatDataset
from .loader import build_dataloader
from .pipelines import PIPELINES, GenerateDistanceMap, LabelAssignment, build_pipeline

__all__ = ["PIPELINES", "LabelAssignment", "GenerateDistanceMap", "build_pipeline", "DATASETS", "BOPDataset", "CocoDataset", "YcbvDataset",
           "ConcatDataset", "RepeatDataset", "MixDataset", "ClassBalancedDataset", "build_dataset", "build_dataloader"]
