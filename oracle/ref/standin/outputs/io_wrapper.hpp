#include "../apk_standin_physics.hpp" // forwarding file: see apk_standin_physics.hpp
