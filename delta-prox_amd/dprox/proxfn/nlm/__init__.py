from .patch_nlm import patch_nlm
