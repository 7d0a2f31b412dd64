// Host check of egc::env_on (egc_amd/csrc/egc_plain.h), THE reading of an on/off switch on the C++ side: prints "<name> on" or
// "<name> off" for every variable named on the command line.  Plain C++, nothing linked from the project and no HIP header;
// tests/test_abi_cpu.py sets the environment and holds the answers to DESIGN.md section 10 and to egc_amd._C.env_flag.
#include <stdio.h>

#include "egc_plain.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) printf("%s %s\n", argv[i], egc::env_on(argv[i]) ? "on" : "off");
  return 0;
}
