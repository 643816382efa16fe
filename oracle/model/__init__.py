"""The Python half of the oracle: rustfst's behaviour restated where the C++ oracle (oracle.cpp) has no such operation,
each rule defined once.  Test infrastructure only, like the rest of oracle/; it imports numpy, the standard library and
oracle_py's TR_DTYPE, never the library under test and nothing from tests/."""
from .weight import *  # noqa: F401,F403
from .props import *  # noqa: F401,F403
from .fst import *  # noqa: F401,F403
from .algorithms import *  # noqa: F401,F403
from .determinize import *  # noqa: F401,F403
from .push import *  # noqa: F401,F403
from .minimize import *  # noqa: F401,F403
from .optimize import *  # noqa: F401,F403
from .rational import *  # noqa: F401,F403
from .top_sort import *  # noqa: F401,F403
