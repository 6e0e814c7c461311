"""Shallow2Deep inference on the device (reference torch_em/shallow2deep): the filter bank, the forest, the enhancer."""
from . import filters
from .shallow2deep_model import RFWithFilters, Shallow2DeepModel, _get_filters
