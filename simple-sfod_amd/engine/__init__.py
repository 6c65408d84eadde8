from .trainer import (BaseTrainer, SourceFreeAdaptiveTeacherTrainer,  # noqa: F401
                      SourceFreeAdaptiveTeacherSingleTrainer, AdaptiveTeacherTrainer, DATrainer, adabn_refinement, test_refinement, get_trainer_class)
from .solver import (FusedSGD, FlatModelState, WarmupCosineLR, WarmupMultiStepLR, build_lr_scheduler,  # noqa: F401
                     build_optimizer)
from . import planted  # noqa: F401
from . import precise_bn  # noqa: F401
from .precise_bn import get_bn_modules, update_bn_stats  # noqa: F401
