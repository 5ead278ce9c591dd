from .inference import InferenceWrapper
from .graph_exec import GraphedEncoder
from .classifier_inference import (ClassifierInferenceWrapper,
                                   save_classifier_artifacts)

__all__ = ["InferenceWrapper", "GraphedEncoder", "ClassifierInferenceWrapper",
           "save_classifier_artifacts"]
