#include "apk_standin.hpp" // forwarding file: see apk_standin.hpp
