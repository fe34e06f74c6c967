"""Model zoo (DSL-built NetParameters + reference solver settings)."""
from .zoo import (MODELS, alexnet, build, caffenet, cifar10_full, cifar10_quick, googlenet, lenet,  # noqa: F401
                  mobilenet, resnet50, resnet_cifar, resnext, resnext50, se_resnet, se_resnet50, solver_for, vgg16)
