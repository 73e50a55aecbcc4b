// strsafe.h -- stand-in for the Win32 header of this name: empty on purpose.  Everything the reference
// host classes use from it is declared in windows.h beside this file (see there).
#pragma once
