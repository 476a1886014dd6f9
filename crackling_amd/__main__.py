"""python -m crackling_amd -c config.ini: crackling_amd.driver."""
import sys

from .driver import main

sys.exit(main())
