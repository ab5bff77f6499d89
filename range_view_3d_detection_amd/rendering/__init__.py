"""Debug panels of the training loop on the device (:mod:`.tensorboard`: the reference's ``rendering/tensorboard.py`` by name)."""
