def __getattr__(name):
    # islpose.SignTrainer / islpose.SignClassifier, imported on first use
    if name == "SignTrainer":
        from .train import SignTrainer
        return SignTrainer
    if name == "WindowAugment":
        from .sign_augment import WindowAugment
        return WindowAugment
    if name == "SignClassifier":
        from .translate import SignClassifier
        return SignClassifier
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
