from .model import model  # noqa: F401
from .eval import latents  # noqa: F401
from .data import device_data  # noqa: F401
